"""Transformer.align end to end on the GPU: a small hybrid model (2 + 2 layers, d 512, T = 64 spectrogram frames, so
T' = 15 encoder frames) aligns three transcripts of different lengths, one of them longer than T'.  The reference is
tests/ctc_align_ref.py in fp64 on the model's own CTC logits copied to the host, under the tolerance rule of
tests/test_gpu_ctc_align_kernels.py (4 x the reference's fp32 error on the score, floored at 1e-5 * max(1, |value|));
the path must equal the reference's wherever the reference's on-path margin is >= 10 x that bound."""
import functools

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R
from tests import ctc_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
V, F_IN, T_IN, D = 250, 80, 64, 512
BOS, EOS, PAD = 1, 2, 4
TRANSCRIPTS = [[17, 93, 93, 200, 8], [5, 249, 31, 77, 120, 64, 12, 180, 41], list(range(10, 30))]   # 5, 9, 20 labels
N_TEXT = 24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def setup():
    """(model, spectrum, text, logits on the host (B, T', V)); computed once."""
    import asrx
    torch.manual_seed(5)
    m = asrx.Transformer(V, F_IN, D, 32, 64, 2, 2, 8, 1024, dropout=0.0, pad_token_id=PAD, eos_token_id=EOS,
                         precision="fp32", ctc=True)
    with torch.no_grad():
        m.ctc_head.weight.mul_(4.0)      # spread the frame posteriors: wider decision margins
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(6)
    spectrum = torch.randn(len(TRANSCRIPTS), 1, F_IN, T_IN, generator=g)
    text = torch.full((len(TRANSCRIPTS), N_TEXT), PAD, dtype=torch.int64)
    for b, tr in enumerate(TRANSCRIPTS):
        row = [BOS] + tr + [EOS]
        text[b, :len(row)] = torch.tensor(row)
    logits = m.ctc_logits(spectrum.to(dev))
    torch.cuda.synchronize()
    assert logits.shape == (len(TRANSCRIPTS), asrx.subsampled(T_IN), V) and logits.shape[1] == 15
    return m, spectrum, text, logits.float().cpu()


def check(a, logits, frames):
    """The alignment `a` of every sample against the reference on `logits` over frames[b] frames."""
    m = setup()[0]
    Tp = logits.shape[1]
    fp, fl, st, en, cf, sc = (t.cpu() for t in a[:6])
    tg, tl = a.targets.cpu(), a.target_lengths.cpu()
    assert fp.shape == (3, Tp) and st.shape == (3, N_TEXT) and sc.shape == (3,)
    for b, tr in enumerate(TRANSCRIPTS):
        assert int(tl[b]) == len(tr) and tg[b, :len(tr)].tolist() == tr      # BOS / EOS / PAD dropped
        x = logits[b].numpy()
        r = R.viterbi(x, tr, m.ctc_blank, frames[b], N_TEXT)
        if not r["feasible"]:
            assert float(sc[b]) == -INF and (fp[b] == -1).all() and (fl[b] == 0).all()
            assert (st[b] == -1).all() and (en[b] == -1).all() and (cf[b] == 0).all()
            continue
        r32 = R.viterbi(x, tr, m.ctc_blank, frames[b], N_TEXT, dtype=np.float32)
        err = abs(r["score"] - r32["score"])
        bound = R.bound(err, r["score"])
        exact = r["margin"] >= 10 * bound
        print(f"sample {b}: T_b {frames[b]}, score {r['score']:.4f}, bound {bound:.2e}, margin {r['margin']:.3e}, "
              f"{'exact' if exact else 'within the bound'}")
        pos = fp[b].numpy()
        assert R.path_is_valid(pos, tr, frames[b])
        total, flp = R.rescore(x, tr, m.ctc_blank, pos, frames[b])
        assert r["score"] - bound <= total <= r["score"] + 1e-9
        assert abs(float(sc[b]) - total) <= bound
        # the sum of frame_logp is the score
        assert abs(float(fl[b].double().sum()) - float(sc[b])) <= bound
        for t in range(Tp):
            assert abs(float(fl[b, t]) - flp[t]) <= R.bound(err, flp[t])
        ws, we, wc = R.spans_of(pos, flp, len(tr), N_TEXT)
        assert st[b].tolist() == ws.tolist() and en[b].tolist() == we.tolist()
        assert all(abs(float(cf[b, u]) - wc[u]) <= R.bound(err, wc[u]) for u in range(N_TEXT))
        if exact:
            assert pos.tolist() == r["frame_pos"].tolist()
    return sc


def test_align_matches_reference_on_the_models_logits():
    m, spectrum, text, logits = setup()
    a = m.align(spectrum.to(dev), text.to(dev))
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in a)
    sc = check(a, logits, [15, 15, 15])
    # 20 labels over 15 frames: no alignment, and the other samples are what they are without it
    assert float(sc[2]) == -INF and torch.isfinite(sc[:2]).all()
    alone = m.align(spectrum[:2].to(dev), text[:2].to(dev))
    # (a batch of two runs other GEMM shapes: equal within the bound, not bit for bit)
    for b in range(2):
        assert abs(float(alone.score[b]) - float(sc[b])) <= 1e-4 * max(1.0, abs(float(sc[b])))
    # an explicit mask that hides the last two labels of sample 1
    mask = (text != PAD).float()
    mask[1, 1 + 7:] = 0
    short = m.align(spectrum.to(dev), text.to(dev), mask.to(dev))
    assert short.target_lengths.tolist() == [5, 7, 20]


def test_input_lengths_are_honoured():
    m, spectrum, text, logits = setup()
    frames = [15, 10, 12]
    a = m.align(spectrum.to(dev), text.to(dev), input_lengths=torch.tensor(frames))
    torch.cuda.synchronize()
    check(a, logits, frames)
    assert (a.frame_pos[1, 10:] == -1).all() and (a.frame_logp[1, 10:] == 0).all()
    assert int(a.end[1, 8]) <= 10


def test_best_path_does_not_beat_the_sum_over_paths():
    """score <= -nll of asrx.CTCLoss on the same logits (the best path is one term of the sum), and the spans map to
    spectrogram frames inside the input."""
    import asrx
    m, spectrum, text, logits = setup()
    a = m.align(spectrum.to(dev), text.to(dev))
    x = m.ctc_logits(spectrum.to(dev)).contiguous()
    nll = asrx.CTCLoss(blank=m.ctc_blank, reduction="none")(x, a.targets, None, a.target_lengths)
    torch.cuda.synchronize()
    for b in range(3):
        s, n = float(a.score[b]), float(nll[b])
        print(f"sample {b}: best path {s:.4f}, log-likelihood {-n:.4f}")
        if b == 2:
            assert s == -INF and n == INF
        else:
            assert s <= -n + 1e-5 * max(1.0, abs(n))
    first, last = asrx.frame_span(a.start.cpu(), a.end.cpu())
    L = len(TRANSCRIPTS[0])
    assert (first[0, :L] >= 0).all() and (last[0, :L] <= T_IN).all() and (first[0, L:] == -1).all()
    # reference check of the helper this test leans on
    assert ctc_ref.collapse([TRANSCRIPTS[0][p] if p >= 0 else m.ctc_blank for p in a.frame_pos[0].tolist()],
                            m.ctc_blank) == TRANSCRIPTS[0]
