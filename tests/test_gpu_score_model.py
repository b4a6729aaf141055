"""Scoring end to end on the GPU: asrx.ErrorRate over the output of every decoder of a small hybrid model (2 + 2
layers, d 512, T = 64 spectrogram frames, so T' = 15 encoder frames; the size of test_gpu_ctc_align_model.py), and
minimum-Bayes-risk ordering through rescore(mbr_scale=...) and asrx.mbr_rerank.

Error counts are integers: they equal tests/edit_ref.py run on the host copies of the same tokens, exactly.  MBR
risks follow the tolerance of tests/test_gpu_edit_kernels.py (4 x the reference's fp32-against-fp64 error, floored at
1e-5 * max(1, |value|)) against the reference computed from the tokens and scores of the mbr_scale=None run, and the
order is compared exactly on the samples whose smallest fp64 risk gap is >= 10 x that bound.  SEED was chosen so that
at least one sample qualifies (recorded in DESIGN.md section 13)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import edit_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
V, F_IN, T_IN, D = 250, 80, 64, 512
BOS, EOS, PAD = 1, 2, 4
SEED = 5
TRANSCRIPTS = [[17, 93, 93, 200, 8], [5, 249, 31, 77, 120, 64, 12, 180, 41], list(range(10, 30)), []]
N_TEXT = 24
DECODERS = ("ctc_greedy", "ctc_beam_search", "beam_search", "rescore")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def setup():
    """(model, spectrum on the device, text on the host); built once."""
    import asrx
    torch.manual_seed(SEED)
    m = asrx.Transformer(V, F_IN, D, 32, 64, 2, 2, 8, 1024, dropout=0.0, pad_token_id=PAD, eos_token_id=EOS,
                         precision="fp32", ctc=True)
    with torch.no_grad():
        m.ctc_head.weight.mul_(4.0)      # spread the frame posteriors, as the alignment test does
    m = m.to(dev).eval()
    spectrum = torch.randn(len(TRANSCRIPTS), 1, F_IN, T_IN, generator=torch.Generator().manual_seed(SEED + 1))
    text = torch.full((len(TRANSCRIPTS), N_TEXT), PAD, dtype=torch.int64)
    for b, tr in enumerate(TRANSCRIPTS):
        row = [BOS] + tr + [EOS]
        text[b, :len(row)] = torch.tensor(row)
    assert m.token_drop_ids() == (BOS, EOS, PAD)
    return m, spectrum.to(dev), text


@functools.lru_cache(maxsize=None)
def decode(name):
    m, spectrum, _ = setup()
    if name == "ctc_greedy":
        return m.ctc_greedy(spectrum)
    if name == "ctc_beam_search":
        return m.ctc_beam_search(spectrum, beam=4, nbest=4)
    if name == "beam_search":
        return m.beam_search(spectrum, beam=3, nbest=3, max_len=8)
    return m.rescore(spectrum, beam=8, nbest=8)


def host_rows(result):
    """(tokens (B, W, cols), lengths per row or None, hypotheses that exist per sample) on the host."""
    if hasattr(result, "scores"):
        return result.tokens.cpu(), None, torch.isfinite(result.scores.cpu()).sum(dim=1).tolist()
    tokens, lengths = result
    return tokens.cpu()[:, None, :], lengths.cpu().tolist(), [1] * tokens.shape[0]


def reference_rates(result, text, drop):
    tokens, lengths, n_hyp = host_rows(result)
    B, W, _ = tokens.shape
    tot = dict(edits=0, sub=0, dele=0, ins=0, ref=0, wrong=0, oracle=0)
    for b in range(B):
        ref = R.sequence(text[b], None, drop)
        al = [R.align(R.sequence(tokens[b, w], None if lengths is None else lengths[b], drop), ref)
              for w in range(n_hyp[b])]
        e, s, d, i, n = al[0]
        tot["edits"] += e
        tot["sub"] += s
        tot["dele"] += d
        tot["ins"] += i
        tot["ref"] += n
        tot["wrong"] += e > 0
        tot["oracle"] += min(a[0] for a in al)
    return tot, B, W


@pytest.mark.parametrize("name", DECODERS)
def test_error_rate_equals_the_reference_on_the_same_tokens(name):
    import asrx
    m, _, text = setup()
    drop = m.token_drop_ids()
    res = decode(name)
    er = asrx.ErrorRate(drop)
    er.update_result(res, text)
    got = er.compute()
    tot, B, W = reference_rates(res, text, drop)
    print(name, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in got.items()})
    assert got["n_edits"] == tot["edits"] and got["n_sub"] == tot["sub"] and got["n_del"] == tot["dele"]
    assert got["n_ins"] == tot["ins"] and got["n_ref"] == tot["ref"] == sum(len(t) for t in TRANSCRIPTS)
    assert got["n_samples"] == B and got["n_wrong"] == tot["wrong"]
    assert got["ter"] == tot["edits"] / tot["ref"] and got["ser"] == tot["wrong"] / B
    assert got["sub"] + got["del"] + got["ins"] == pytest.approx(got["ter"], rel=1e-12)
    if W > 1:
        assert got["n_oracle_edits"] == tot["oracle"] and got["oracle_ter"] == tot["oracle"] / tot["ref"]
        assert got["oracle_ter"] <= got["ter"]
    else:
        assert "oracle_ter" not in got
    # against its own 1-best as the transcript: no edits; two updates accumulate
    tokens, lengths, _ = host_rows(res)
    own = tokens[:, 0, :].clone()
    if lengths is not None:                       # ctc_greedy: the fill past the length is the blank already
        assert all((own[b, n:] == PAD).all() for b, n in enumerate(lengths))
    er.reset()
    er.update_result(res, own)
    er.update_result(res, own.to(dev))
    zero = er.compute()
    assert zero["n_edits"] == 0 and zero["n_wrong"] == 0 and zero["n_samples"] == 2 * B and zero["ser"] == 0.0
    assert zero["ter"] == 0.0 if zero["n_ref"] else math.isnan(zero["ter"])


def test_update_with_plain_rows_and_lengths():
    """ErrorRate.update on 1-best rows with explicit lengths, and asrx.edit_distance on the same rows."""
    import asrx
    m, _, text = setup()
    tokens, lengths = decode("ctc_greedy")
    er = asrx.ErrorRate(m.token_drop_ids())
    er.update(tokens, text.to(dev), lengths)
    got = er.compute()
    e = asrx.edit_distance(tokens, text, lengths, drop=m.token_drop_ids())
    assert got["n_edits"] == int(e.dist.sum()) and got["n_ref"] == int(e.ref_len.sum())
    want = [R.align(R.sequence(tokens[b].cpu(), int(lengths[b]), (BOS, EOS, PAD)), TRANSCRIPTS[b])
            for b in range(len(TRANSCRIPTS))]
    assert e.dist.tolist() == [a[0] for a in want] and e.ins.tolist() == [a[3] for a in want]


def labels_of(tokens_row, length):
    """The labels of a rescore row (BOS, labels, EOS...; length counts the EOS; 0: no hypothesis)."""
    return tuple(int(t) for t in tokens_row[1:int(length)]) if int(length) > 0 else None


def mbr_reference(base, b, scale):
    """From the mbr_scale=None result of sample b: (labels per slot, fp64 risks, live, bound, gap, order)."""
    W = base.tokens.shape[1]
    hyps = [labels_of(base.tokens[b, w], base.lengths[b, w]) for w in range(W)]
    n = sum(h is not None for h in hyps)
    assert all(h is not None for h in hyps[:n]) and len(set(hyps[:n])) == n      # dead slots last, all distinct
    dist = np.full((W, W), -1, dtype=np.int64)
    dist[:n, :n] = R.cross_distances([list(h) for h in hyps[:n]])
    r64, live, bnd, gap = R.mbr_check(dist, base.scores[b].numpy(), n, scale)
    return hyps, r64, live, bnd, gap, R.mbr_order(r64)


def check_mbr(base, got, scale, what):
    """`got`, an MBR ordering of `base`: the same hypotheses with their scores, risks within the bound, the order exact
    where the gaps allow.  Returns the number of samples whose order was compared."""
    B, W = base.scores.shape
    exact, worst = 0, 0.0
    for b in range(B):
        hyps, r64, live, bnd, gap, order = mbr_reference(base, b, scale)
        n = int(live.sum())
        ghyps = [labels_of(got.tokens[b, w], got.lengths[b, w]) for w in range(W)]
        # the same multiset of hypotheses, each with its scores
        assert sorted(h for h in ghyps if h is not None) == sorted(h for h in hyps if h is not None)
        assert all(h is None for h in ghyps[n:]) and np.isposinf(got.risks[b, n:].numpy()).all()
        for w in range(n):
            k = hyps.index(ghyps[w])
            assert got.scores[b, w].item() == base.scores[b, k].item()
            assert got.att_scores[b, w].item() == base.att_scores[b, k].item()
            assert got.ctc_scores[b, w].item() == base.ctc_scores[b, k].item()
            assert torch.equal(got.tokens[b, w], base.tokens[b, k]) and got.lengths[b, w] == base.lengths[b, k]
            err = abs(float(got.risks[b, w]) - r64[k])
            worst = max(worst, err / bnd[k])
            assert err <= bnd[k], (what, b, w, err, bnd[k])
        risks = got.risks[b, :n].tolist()
        assert all(x <= y + 2 * bnd.max() for x, y in zip(risks, risks[1:]))          # ascending within the bound
        qualifies = n >= 2 and gap >= 10 * bnd.max()
        print(f"{what} sample {b}: {n} hypotheses, smallest risk gap {gap:.3e}, bound {bnd.max():.2e}, "
              f"{'order exact' if qualifies else 'within the bound'}; MBR first = score rank {order[0]}")
        if qualifies:
            exact += 1
            assert ghyps[:n] == [hyps[k] for k in order[:n]], (what, b)
    print(f"{what}: worst risk error / bound {worst:.3f}, order compared on {exact} of {B} samples")
    return exact


def test_rescore_mbr_scale_and_mbr_rerank():
    import asrx
    m, spectrum, _ = setup()
    base = decode("rescore")
    assert base.risks is None and base.tokens.shape[:2] == (len(TRANSCRIPTS), 8)
    got = m.rescore(spectrum, beam=8, nbest=8, mbr_scale=1.0)
    assert isinstance(got, asrx.RescoreResult) and got.risks.shape == base.scores.shape
    assert check_mbr(base, got, 1.0, "rescore(mbr_scale=1)") >= 1
    # the same ordering from the finished result: rows BOS, labels, EOS fill -> drop BOS, stop at EOS.  (A CTC label
    # that is itself the EOS or BOS id would be read differently there; none occurs under this seed.)
    n_live = int(torch.isfinite(base.scores).sum())
    assert not any(t in (BOS, EOS) for b in range(base.tokens.shape[0]) for w in range(8)
                   for t in (labels_of(base.tokens[b, w], base.lengths[b, w]) or ()))
    again = asrx.mbr_rerank(base, scale=1.0, drop=(BOS,), stop=EOS)
    assert isinstance(again, asrx.RescoreResult) and int(torch.isfinite(again.risks).sum()) == n_live
    assert check_mbr(base, again, 1.0, "mbr_rerank") >= 1
    # scale 0 through the model entry: the medoid of each sample first
    med = m.rescore(spectrum, beam=8, nbest=8, mbr_scale=0.0)
    check_mbr(base, med, 0.0, "rescore(mbr_scale=0)")
    # nbest < beam keeps the head of the MBR order over all `beam` hypotheses
    top = m.rescore(spectrum, beam=8, nbest=2, mbr_scale=1.0)
    assert torch.equal(top.tokens, got.tokens[:, :2]) and torch.equal(top.risks, got.risks[:, :2])
    # a BeamResult (the first pass alone: labels, blank fill) gives an MbrResult
    first = decode("ctc_beam_search")
    r = asrx.mbr_rerank(first, scale=1.0, drop=(PAD,))
    assert isinstance(r, asrx.MbrResult) and r.tokens.shape == first.tokens.shape
    for b in range(first.tokens.shape[0]):
        assert sorted(map(tuple, r.tokens[b].tolist())) == sorted(map(tuple, first.tokens[b].tolist()))
