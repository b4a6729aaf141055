"""Padded batches on the GPU: Transformer(..., mask_padding=True) with per-utterance lengths against the
oracle run on every utterance ALONE, trimmed to its length, and against itself with other padding.

Model: d 512, 8 heads (dh 64: the fused kernels), 2 + 2 layers, vocab 250, L = 16, det_params, B = 3.  Geometries
(spectrogram frames -> encoder frames T'), and the program each masked bf16 attention takes (fp32 always takes the
materialised-scores program with asrx_softmax_fwd mode 1):
  G1  T   64: 64, 40, 23     -> 15, 9, 5       encoder and cross-attention: resident forward / backward <1>
  G2  T  600: 600, 333, 130  -> 149, 82, 31    T' % 4 = 1: the encoder on attn_fwd_stream_kernel<1> (two chunks) and
                                               attn_bwd_res_kernel<1, 8>, the last validity word partial;
                                               cross-attention (16 queries): resident <1>
  G3  T 1100: 1100, 700, 130 -> 274, 174, 31   T' % 4 = 2, T' > 256: encoder and cross-attention on
                                               attn_fwd_stream_kernel<1>, the key-block backward <1, 8, true>
  G4  T  611: 611, 333, 130  -> 152, 82, 31    T' % 4 = 0: the encoder on attn_fwd_stream_kernel<1> at 128 < Lk <= 256
                                               and attn_bwd_res_kernel<1, 8>; two utterances leave whole 32-key tiles
                                               dead; cross-attention: resident <1>
  G5  T 1107: 1107, 700, 130 -> 276, 174, 31   T' % 4 = 0, T' > 256: encoder and cross-attention on
                                               attn_fwd_stream_kernel<1>, the key-block backward <1, 8, true> with the
                                               second 256-key block wholly dead for two utterances
G1 - G3 are the issue's.  G2 and G3 took the materialised-scores program while the streamed kernel clipped the last
validity word; kernels.length_mask's rows are a multiple of 4 bytes apart, so all five stream now.
The padding is 10 * N(0, 1).  Bounds: fp32 relerr < 1e-3 (test_forward_c2_fp32_vs_oracle's); bf16 relerr <= BF16_FACTOR
x the oracle's own bf16-autocast error (the first rule of tests/bf16_check.py; 48 positions cannot carry its argmax
rule); gradients by test_train_grads_micro's procedure and fp32 bound; independence of the padding bit for bit."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.ref_model import OracleConfig, det_params, forward as oracle_forward, synthetic_batch
from tests import lengths_ref
from tests.bf16_check import BF16_FACTOR, relerr

pytestmark = pytest.mark.gpu
dev = "cuda"
CFG = OracleConfig(vocab_size=250, input_dim=80, d_model=512, dec_len=16, enc_len=300, n_enc=2, n_dec=2, n_heads=8,
                   ff_dim=1024, dropout=0.0)
B, L = 3, 16
GEOS = {"G1": (64, (64, 40, 23), (15, 9, 5)), "G2": (600, (600, 333, 130), (149, 82, 31)),
        "G3": (1100, (1100, 700, 130), (274, 174, 31)), "G4": (611, (611, 333, 130), (152, 82, 31)),
        "G5": (1107, (1107, 700, 130), (276, 174, 31))}
# every geometry in both precisions but G4 and G5, which exist for the bf16 kernels (fp32 runs at G2 and G3 what it
# would run there)
GEO_PRECISIONS = [(g, p) for g in ("G1", "G2", "G3") for p in ("fp32", "bf16")] + [("G4", "bf16"), ("G5", "bf16")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def params():
    return det_params(CFG, 0)


def build(precision, dropout=0.0, ctc=False, mask_padding=True):
    import asrx
    torch.manual_seed(7)    # (the CTC head is not among the oracle's parameters: its own init)
    m = asrx.Transformer(CFG.vocab_size, CFG.input_dim, CFG.d_model, CFG.dec_len, CFG.enc_len, CFG.n_enc, CFG.n_dec,
                         CFG.n_heads, CFG.ff_dim, dropout=dropout, pad_token_id=CFG.pad_id, eos_token_id=CFG.eos_id,
                         precision=precision, ctc=ctc, mask_padding=mask_padding)
    sd = m.state_dict()
    sd.update(params())
    m.load_state_dict(sd)
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def batch(geo, lens=None):
    """(spectrum with garbage padding, the same with zero padding, text (B, L+1), mask) on the host."""
    T, lengths, enc = GEOS[geo]
    lengths = lens or lengths
    if lens is None:
        assert tuple(int(v) for v in lengths_ref.rows(lengths, 1 << 20, 2)) == enc
    s, t, k = synthetic_batch(CFG, B, T, L + 1, seed=1234)
    g = torch.Generator().manual_seed(99)
    junk, zero = s.clone(), s.clone()
    for b, n in enumerate(lengths):
        junk[b, :, :, n:] = 10.0 * torch.randn(junk[b, :, :, n:].shape, generator=g)
        zero[b, :, :, n:] = 0.0
    return junk, zero, t, k


def enc_lens(geo):
    return torch.tensor(GEOS[geo][2], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def oracle(geo, b):
    """Utterance b alone, trimmed: (logits (L, V), encoder (T'_b, d)) in fp32 and under bf16 autocast."""
    _, lengths, enc = GEOS[geo]
    _, zero, t, k = batch(geo)
    s = zero[b:b + 1, :, :, :lengths[b]]
    with torch.no_grad():
        lg, e = oracle_forward(params(), s, t[b:b + 1, :-1], k[b:b + 1, :-1], CFG, False, return_encoder=True)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            lg16, e16 = oracle_forward(params(), s, t[b:b + 1, :-1], k[b:b + 1, :-1], CFG, False, return_encoder=True)
    assert e.shape[1] == enc[b]
    return lg[0], e[0], lg16[0].float(), e16[0].float()


def assert_close(x, ref, ref16, precision, label):
    e = relerr(x, ref)
    if precision == "fp32":
        print(f"{label}: fp32 rel err {e:.3e} (bound 1e-3)")
        assert e < 1e-3, (label, e)
    else:
        e16 = relerr(ref16, ref)
        print(f"{label}: bf16 rel err {e:.3e} (reference bf16-autocast path {e16:.3e})")
        assert e <= BF16_FACTOR * e16, (label, e, e16)


def same(a, b, label):
    """Bit equality of two results: tensors, or tuples / lists of them (None fields equal None)."""
    if a is None or b is None:
        assert a is None and b is None, label
    elif torch.is_tensor(a):
        assert a.shape == b.shape and torch.equal(a, b), label
    else:
        assert len(a) == len(b), label
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{label}[{i}]")


# ------------------------------------------------------------------------------------------- the kernel

@pytest.mark.parametrize("subsample", [0, 2])
def test_length_mask_kernel(subsample):
    """asrx_length_mask against tests/lengths_ref.py, exactly; the columns behind T keep their sentinel; each output may
    be left out."""
    import asrx
    from asrx._lib import call
    from asrx.kernels import stream
    lengths = [-3, 0, 6, 7, 130, 1100, 5000]
    T, vb, n = 274, 288, 7
    ref_len, ref_valid = lengths_ref.length_mask(lengths, T, subsample)
    dl = torch.tensor(lengths, dtype=torch.int32, device=dev)
    for want_len, want_valid in ((True, True), (True, False), (False, True)):
        enc = torch.full((n,), -77, dtype=torch.int32, device=dev)
        valid = torch.full((n, vb), 0xA5, dtype=torch.uint8, device=dev)
        call("asrx_length_mask", dl.data_ptr(), n, T, subsample, enc.data_ptr() if want_len else None,
             valid.data_ptr() if want_valid else None, vb, stream())
        torch.cuda.synchronize()
        if want_len:
            assert enc.cpu().numpy().tolist() == ref_len.tolist()
        else:
            assert (enc == -77).all()
        if want_valid:
            assert np.array_equal(valid[:, :T].cpu().numpy(), ref_valid)
            assert (valid[:, T:] == 0xA5).all()
        else:
            assert (valid == 0xA5).all()
    enc, valid = asrx.kernels.length_mask(dl, T, subsample)
    assert enc.cpu().numpy().tolist() == ref_len.tolist() and np.array_equal(valid.cpu().numpy(), ref_valid)


# ------------------------------------------------------------------------------------------- forward vs the oracle

@pytest.mark.parametrize("geo,precision", GEO_PRECISIONS)
def test_logits_vs_oracle_of_each_utterance_alone(geo, precision):
    m = build(precision).eval()
    junk, _, t, k = batch(geo)
    with torch.no_grad():
        logits = m(junk.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev), input_lengths=enc_lens(geo)).float().cpu()
    refs = [oracle(geo, b) for b in range(B)]
    assert torch.isfinite(logits).all()
    assert_close(logits, torch.stack([r[0] for r in refs]), torch.stack([r[2] for r in refs]), precision,
                 f"{geo} logits")


@pytest.mark.parametrize("geo,precision", GEO_PRECISIONS)
def test_encoder_rows_vs_oracle_of_each_utterance_alone(geo, precision):
    """Encoder.forward(x, input_lengths=): its valid rows, stacked, against the oracle's encoder outputs.  G2 (149 rows)
    and G3 (274) are no multiples of 4: the full-length utterance pins the last Lk % 4 keys, which the streamed kernel's
    word-wise read of the validity bytes once dropped (the word that holds byte Lk - 1 was clipped by the descriptor's
    range; tests/test_gpu_attention_keymask.py holds the kernel itself to that); with them dropped G3-bf16 read 4.57e-03
    against its bound of 4.17e-03.  G4 (152) and G5 (276) are multiples of 4: the same check of the key mask with whole
    32-key tiles and a whole 256-key block dead."""
    m = build(precision).eval()
    junk, _, t, k = batch(geo)
    el = enc_lens(geo)
    with torch.no_grad():
        enc = m.encoder(m.input_layer(junk.to(dev)), input_lengths=el.to(dev)).float().cpu()
    refs = [oracle(geo, b) for b in range(B)]
    assert torch.isfinite(enc).all()
    rows = torch.cat([enc[b, :int(el[b])] for b in range(B)])
    assert_close(rows, torch.cat([r[1] for r in refs]), torch.cat([r[3] for r in refs]), precision,
                 f"{geo} encoder rows")


# ------------------------------------------------------------------------------------------- gradients vs the oracle

@pytest.mark.parametrize("geo", ["G1", "G3"])
def test_grads_vs_oracle_of_each_utterance_alone(geo):
    """fp32, dropout 0, the autograd path, mean CE over the B * L positions; the reference: the per-utterance CE sums of
    the oracle on trimmed inputs, over B * L, backpropagated once.  test_train_grads_micro's comparison."""
    import asrx
    tol = 1e-3
    _, lengths, _ = GEOS[geo]
    junk, zero, t, k = batch(geo)
    m = build("fp32").train()
    logits = m(junk.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev), input_lengths=enc_lens(geo))
    loss = F.cross_entropy(logits.transpose(1, 2), t[:, 1:].to(dev))
    loss.backward()
    P = {key: v.clone().requires_grad_(True) for key, v in params().items()}
    total = 0.0
    for b in range(B):
        lg = oracle_forward(P, zero[b:b + 1, :, :, :lengths[b]], t[b:b + 1, :-1], k[b:b + 1, :-1], CFG, False)
        total = total + F.cross_entropy(lg.transpose(1, 2), t[b:b + 1, 1:], reduction="sum")
    ref_loss = total / (B * L)
    ref_loss.backward()
    print(f"{geo}: loss {float(loss.detach()):.6f}, reference {float(ref_loss.detach()):.6f}")
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < tol * abs(float(ref_loss.detach()))
    twin = asrx.Transformer(CFG.vocab_size, CFG.input_dim, CFG.d_model, CFG.dec_len, CFG.enc_len, CFG.n_enc, CFG.n_dec,
                            CFG.n_heads, CFG.ff_dim, dropout=0.0, pad_token_id=CFG.pad_id, eos_token_id=CFG.eos_id)
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), twin.named_parameters()):
            assert n1 == n2
            p2.copy_(p1.grad.cpu() if p1.grad is not None else torch.zeros_like(p2))
    gsd = twin.state_dict()
    ref = {key: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for key, v in P.items()}
    gmax = max(float(g.abs().max()) for g in ref.values())
    worst = 0.0
    for key, g in ref.items():
        assert torch.isfinite(gsd[key]).all(), key
        if float(g.abs().max()) < 1e-6 * gmax:
            # mathematically zero gradient: an absolute match at the global scale
            assert float((gsd[key].double() - g.double()).abs().max()) < tol * 1e-2 * gmax, key
            continue
        e = relerr(gsd[key], g)
        worst = max(worst, e)
        assert e < tol, (key, e)
    print(f"{geo}: worst gradient rel err {worst:.3e} over {len(ref)} parameters")


# ------------------------------------------------------------------------------------------- padding content

@pytest.mark.parametrize("geo,precision", GEO_PRECISIONS)
def test_logits_do_not_depend_on_the_padding(geo, precision):
    m = build(precision).eval()
    junk, zero, t, k = batch(geo)
    out = []
    with torch.no_grad():
        for s in (junk, zero, junk):
            out.append(m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev), input_lengths=enc_lens(geo)))
    assert torch.equal(out[0], out[2]), "the forward is not reproducible on identical input"
    assert torch.equal(out[0], out[1])
    # and without the lengths the padding does reach the logits: the test above is not vacuous
    with torch.no_grad():
        a, b = (m(s.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev)) for s in (junk, zero))
    assert not torch.equal(a[1:], b[1:])


@pytest.mark.parametrize("geo", ["G1", "G2"])
def test_decodes_do_not_depend_on_the_padding(geo):
    m = build("bf16", ctc=True).eval()
    junk, zero, t, k = batch(geo)
    el = enc_lens(geo)
    bos = torch.full((B, 1), 1, dtype=torch.int32, device=dev)

    def rescored(r):
        return tuple(r) + (r.att_scores, r.ctc_scores)

    calls = {
        "evaluate": lambda s: m.evaluate(s, bos, input_lengths=el),
        "beam_search": lambda s: m.beam_search(s, beam=4, input_lengths=el),
        "beam_search joint": lambda s: m.beam_search(s, beam=4, ctc_weight=0.3, input_lengths=el),
        "rescore": lambda s: rescored(m.rescore(s, beam=4, input_lengths=el)),
        "ctc_beam_search": lambda s: m.ctc_beam_search(s, input_lengths=el),
        "ctc_greedy": lambda s: m.ctc_greedy(s, input_lengths=el),
        "align": lambda s: tuple(m.align(s, t.to(dev), input_lengths=el)),
    }
    for name, fn in calls.items():
        a, b = fn(junk.to(dev)), fn(zero.to(dev))
        torch.cuda.synchronize()
        same(a, b, f"{geo} {name}")


def run_trainer(geo, spectra, lengths, graph, *, steps=6, dropout=0.1, mask_padding=True, precision="bf16",
                ctc_weight=0.3):
    """`steps` Trainer steps on spectra[i % len] with lengths[i % len] (None: no lengths): (flat parameters, losses)."""
    from asrx import functions, kernels as K
    from asrx.train import Trainer
    _, _, t, k = batch(geo)
    m = build(precision, dropout=dropout, ctc=True, mask_padding=mask_padding).train()
    torch.manual_seed(11)                 # the dropout seeds of the eager steps ...
    functions._SEED_FALLBACK.clear()      # ... and of the capture, the same in every run
    K.set_seed_offset(0)
    tr = Trainer(m, lr=1e-3, graph=graph, ctc_weight=ctc_weight)
    t, k = t.to(dev), k.to(dev)
    losses = []
    for i in range(steps):
        n = lengths[i % len(lengths)]
        losses.append(float(tr.step(spectra[i % len(spectra)].to(dev), t, k,
                                    input_lengths=None if n is None else torch.tensor(n, dtype=torch.int32))))
    torch.cuda.synchronize()
    assert (tr._cap is not None) == (graph and precision == "bf16")
    K.set_seed_offset(0)
    return tr.store.flat.clone(), losses


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("geo", ["G1", "G3", "G4", "G5"])
def test_training_does_not_depend_on_the_padding(geo, graph):
    """6 steps, bf16, dropout 0.1, ctc_weight 0.3: every parameter bit for bit."""
    junk, zero, _, _ = batch(geo)
    lengths = GEOS[geo][1]
    pa, la = run_trainer(geo, [junk], [lengths], graph)
    pb, lb = run_trainer(geo, [zero], [lengths], graph)
    assert torch.isfinite(pa).all() and la == lb
    assert torch.equal(pa, pb)


# ------------------------------------------------------------------------------------------- trainer

@pytest.mark.parametrize("geo", ["G1", "G3"])
def test_graph_steps_equal_eager_steps_with_changing_lengths(geo):
    """Lengths that rotate every step reach the replay through the static lengths buffer and the captured
    asrx_length_mask launch.  Dropout 0: graph and eager steps draw their dropout seeds differently."""
    junk, _, _, _ = batch(geo)
    n = GEOS[geo][1]
    rot = [n, n[1:] + n[:1], n[2:] + n[:2]]
    pe, le = run_trainer(geo, [junk], rot, False, dropout=0.0)
    pg, lg = run_trainer(geo, [junk], rot, True, dropout=0.0)
    assert le == lg and len(set(le[:3])) == 3
    assert torch.equal(pe, pg)


@pytest.mark.parametrize("graph", [False, True])
def test_feature_off_or_without_lengths_is_the_step_as_before(graph):
    junk, _, _, _ = batch("G1")
    n = GEOS["G1"][1]
    base, lb = run_trainer("G1", [junk], [None], graph, steps=4, dropout=0.0, mask_padding=False)
    off, lo = run_trainer("G1", [junk], [n], graph, steps=4, dropout=0.0, mask_padding=False)
    nol, ln = run_trainer("G1", [junk], [None], graph, steps=4, dropout=0.0, mask_padding=True)
    on, _ = run_trainer("G1", [junk], [n], graph, steps=4, dropout=0.0, mask_padding=True)
    assert lb == lo == ln and torch.equal(base, off) and torch.equal(base, nol)
    assert not torch.equal(base, on)


def test_ctc_term_runs_over_each_utterances_own_frames():
    """Step 1's hybrid loss (fp32, dropout 0, eager) is (1 - w) * CE + w * CTC(input_lengths = the encoder lengths) of
    the model's own logits, within the fp32 bound; CTC over all T' frames would miss it."""
    import asrx
    from asrx import kernels as K
    from asrx.train import Trainer
    geo, w = "G2", 0.3
    junk, _, t, k = batch(geo)
    el = enc_lens(geo)
    m = build("fp32", ctc=True).train()
    s, t, k = junk.to(dev), t.to(dev), k.to(dev)
    with torch.no_grad():
        logits = m(s, t[:, :-1], k[:, :-1], input_lengths=el)
        ce = F.cross_entropy(logits.transpose(1, 2), t[:, 1:])
        cl = m.ctc_logits(s, input_lengths=el).contiguous()
        tgt, tl = K.ctc_targets(t, k, [1, CFG.eos_id, CFG.pad_id], m.ctc_blank)
        crit = asrx.CTCLoss(blank=m.ctc_blank, reduction="mean", zero_infinity=True)
        ctc = crit(cl, tgt, el.to(dev), tl)
        ctc_all = crit(cl, tgt, None, tl)
    want, other = float((1 - w) * ce + w * ctc), float((1 - w) * ce + w * ctc_all)
    tr = Trainer(m, lr=1e-3, graph=False, ctc_weight=w)
    loss = float(tr.step(s, t, k, input_lengths=torch.tensor(GEOS[geo][1])))
    print(f"hybrid loss {loss:.6f}, expected {want:.6f} (CE {float(ce):.6f}, CTC {float(ctc):.6f}; over all frames "
          f"{other:.6f})")
    assert abs(loss - want) < 1e-3 * abs(want)
    assert abs(other - want) > 1e-2 * abs(want)


# ------------------------------------------------------------------------------------------- decode vs alone

def test_beam_search_of_the_batch_is_that_of_each_utterance_alone():
    """G1, fp32, beam 4: the tokens of the utterance decoded alone (B = 1, trimmed), its score within 1e-3 relative;
    the B = 1 run's best two hypotheses are further apart than that."""
    m = build("fp32").eval()
    junk, zero, _, _ = batch("G1")
    _, lengths, _ = GEOS["G1"]
    r = m.beam_search(junk.to(dev), beam=4, input_lengths=enc_lens("G1"))
    for b in range(B):
        alone = m.beam_search(zero[b:b + 1, :, :, :lengths[b]].to(dev), beam=4, nbest=2)
        s0, s1 = float(alone.scores[0, 0]), float(alone.scores[0, 1])
        print(f"utterance {b}: alone {s0:.5f} / runner-up {s1:.5f}, in the batch {float(r.scores[b, 0]):.5f}")
        assert s0 - s1 > 1e-3 * abs(s0), (b, s0, s1)
        n = int(alone.lengths[0, 0])
        assert int(r.lengths[b, 0]) == n
        assert r.tokens[b, 0, :1 + n].tolist() == alone.tokens[0, 0, :1 + n].tolist()
        assert abs(float(r.scores[b, 0]) - s0) < 1e-3 * abs(s0)


# ------------------------------------------------------------------------------------------- degenerate lengths

def test_degenerate_lengths_stay_finite():
    """G1 with 64, 6 and 0 spectrogram frames (15, 0, 0 encoder frames): finite everywhere, utterance 0 as the oracle's,
    a training step leaves finite parameters."""
    lens = (64, 6, 0)
    junk, _, t, k = batch("G1", lens)
    el = torch.tensor(lengths_ref.rows(lens, 15, 2))
    assert el.tolist() == [15, 0, 0]
    for precision in ("fp32", "bf16"):
        m = build(precision, ctc=True).eval()
        with torch.no_grad():
            logits = m(junk.to(dev), t[:, :-1].to(dev), k[:, :-1].to(dev), input_lengths=el).float().cpu()
        assert torch.isfinite(logits).all()
        ref = oracle("G1", 0)
        assert_close(logits[0], ref[0], ref[2], precision, "degenerate, utterance 0")
        r = m.beam_search(junk.to(dev), beam=4, ctc_weight=0.3, input_lengths=el)
        assert torch.isfinite(r.scores[0]).all()
    p, losses = run_trainer("G1", [junk], [lens], False, steps=1)
    assert torch.isfinite(p).all() and np.isfinite(losses).all()
