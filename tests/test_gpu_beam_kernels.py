"""asrx_beam_step and asrx_gather_rows on the GPU against fp64 torch on the CPU (tests/beam_ref.py).

beam_step: tokens, parents, source rows, flags, lengths and the live count must match exactly, scores within
rtol = atol = 1e-5 (fp32 logsumexp over <= 5400 terms plus two additions: a few 1e-6 at these magnitudes).  Exact
selection needs the reference's own margins to exceed that error, so every random case first asserts that its fp64
gaps between consecutive kept candidates, and to the first one dropped, are >= 1e-4 (seeds are fixed below)."""
import pytest
import torch

from tests import beam_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
EOS = 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


def K():
    from asrx import kernels
    return kernels


def run_step(logits, score, fin, length, V, eos=EOS, cur=True):
    """logits [B*W, ld] fp32, score / fin / length [B, W] (CPU) -> dict of CPU outputs shaped [B, W]."""
    B, W = score.shape
    R = B * W
    lg = logits.to(dev)
    si, fi, li = (score.reshape(R).float().to(dev), fin.reshape(R).to(torch.uint8).to(dev),
                  length.reshape(R).to(torch.int32).to(dev))
    keep = [t.clone() for t in (lg, si, fi, li)]
    so, fo, lo = torch.empty_like(si), torch.empty_like(fi), torch.empty_like(li)
    tok = torch.full((R,), -7, dtype=torch.int64, device=dev)
    parent = torch.full((R,), -7, dtype=torch.int32, device=dev)
    src_row = torch.full((R,), -7, dtype=torch.int32, device=dev)
    cur_t = torch.full((R,), -7, dtype=torch.int64, device=dev) if cur else None
    n_live = torch.zeros(1, dtype=torch.int32, device=dev)
    K().beam_step(lg, V, B, W, eos, (si, fi, li), (so, fo, lo), tok, parent, src_row, cur=cur_t, n_live=n_live)
    torch.cuda.synchronize()
    for a, b in zip(keep, (lg, si, fi, li)):          # inputs are read only (bitwise: NaN and inf included)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    out = dict(score=so, tok=tok, parent=parent, src_row=src_row, fin=fo, len=lo)
    out = {k: v.cpu().view(B, W) for k, v in out.items()}
    out["n_live"] = int(n_live)
    if cur:
        assert torch.equal(cur_t.cpu().view(B, W), out["tok"])
    return out


def check(out, ref):
    for k in ("tok", "parent", "src_row", "len"):
        assert torch.equal(out[k].long(), ref[k].long()), k
    assert torch.equal(out["fin"].bool(), ref["fin"]), "fin"
    assert out["n_live"] == ref["n_live"]
    assert torch.allclose(out["score"].double(), ref["score"], rtol=1e-5, atol=1e-5)
    W = out["parent"].shape[1]
    assert int(out["parent"].min()) >= 0 and int(out["parent"].max()) < W


# seeds of the random cases whose default seed leaves an fp64 margin under 1e-4 (case -> seed)
SEEDS = {(2100, 2104, 8, 3): 1}      # (its default seed: 5.1e-5)


def make_case(V, ld, W, B):
    """3 * randn logits with +inf in the padding columns; running scores around -5; a finished beam per sample
    once W >= 3 (two once W >= 8), one beam with a -inf score once W >= 2; the last of three samples in the
    step-0 state (score [0, -inf, ...], nothing finished, lengths 0)."""
    g = torch.Generator().manual_seed(SEEDS.get((V, ld, W, B), 1000 * V + 10 * W + B))
    logits = 3 * torch.randn(B * W, ld, generator=g)
    logits[:, V:] = INF
    score = 2 * torch.randn(B, W, generator=g) - 5
    fin = torch.zeros(B, W, dtype=torch.bool)
    length = torch.randint(1, 9, (B, W), generator=g)
    if W >= 3:
        fin[:, 1] = True
    if W >= 8:
        fin[:, W - 2] = True
    if W >= 2:
        score[0, W - 1] = -INF
    if B == 3:
        score[2] = -INF
        score[2, 0] = 0.0
        fin[2] = False
        length[2] = 0
    return logits, score, fin, length


# (V, ld): the four required shapes, then the LDS limit (W * V = 16128 candidates) from both sides and shapes that
# re-read the logits in every round
SHAPES = [(5, 8), (250, 256), (257, 320), (1000, 1000)]
BEYOND = [(1008, 1008, 16, 1), (1009, 1012, 16, 1), (1030, 1032, 16, 3), (2100, 2104, 8, 3), (5000, 5000, 3, 1),
          (5400, 5401, 3, 3)]


CASES = [(V, ld, W, B) for V, ld in SHAPES for W in (1, 3, 8, 16) for B in (1, 3)] + BEYOND


@pytest.mark.parametrize("V,ld,W,B", CASES)
def test_beam_step_random(V, ld, W, B):
    logits, score, fin, length = make_case(V, ld, W, B)
    ref = beam_ref.beam_step(logits.view(B, W, ld), score, fin, length, EOS, V)
    assert ref["gap"] >= 1e-4, f"fp64 margin {ref['gap']:.2e}: choose another seed for this case"
    check(run_step(logits, score, fin, length, V, cur=W != 3), ref)      # (W = 3: without the optional cur)


@pytest.mark.parametrize("V,ld,W", [(5, 8, 3), (250, 256, 16), (16, 16, 16), (1100, 1104, 16)])
def test_beam_step_all_equal_takes_flat_index_order(V, ld, W):
    """Every logit and every score equal: all W * V candidates tie, the slots are flat indices 0 .. W-1."""
    B = 2
    logits = torch.full((B * W, ld), 0.75)
    logits[:, V:] = INF
    score = torch.full((B, W), -1.5)
    out = run_step(logits, score, torch.zeros(B, W, dtype=torch.bool), torch.ones(B, W, dtype=torch.int64), V)
    assert torch.equal(out["parent"].long(), torch.zeros(B, W, dtype=torch.int64))
    assert torch.equal(out["tok"], torch.arange(W).expand(B, W))
    assert torch.equal(out["src_row"].long(), (torch.arange(B) * W)[:, None].expand(B, W))
    assert torch.equal(out["len"].long(), torch.full((B, W), 2))
    assert torch.equal(out["fin"].bool(), out["tok"] == EOS)
    assert out["n_live"] == B * (W - (1 if W > EOS else 0))
    assert float((out["score"] - out["score"][0, 0]).abs().max()) == 0.0
    check(out, beam_ref.beam_step(logits.view(B, W, ld), score, torch.zeros(B, W, dtype=torch.bool), torch.ones(B, W),
                                  EOS, V))


def test_beam_step_more_beams_than_tokens_at_step_zero():
    """V = 5, W = 8, step 0: the root beam's five finite candidates come first, then -inf slots in flat-index
    order, i.e. beam 1 with tokens 0, 1, 2."""
    V, ld, W, B = 5, 8, 8, 2
    logits = 3 * torch.randn(B * W, ld, generator=torch.Generator().manual_seed(3))
    logits[:, V:] = INF
    score = torch.full((B, W), -INF)
    score[:, 0] = 0.0
    fin, length = torch.zeros(B, W, dtype=torch.bool), torch.zeros(B, W, dtype=torch.int64)
    out = run_step(logits, score, fin, length, V)
    ref = beam_ref.beam_step(logits.view(B, W, ld), score, fin, length, EOS, V)
    assert ref["gap"] >= 1e-4
    check(out, ref)
    for b in range(B):
        order = torch.sort(logits[b * W, :V], descending=True, stable=True).indices
        assert out["parent"][b].tolist() == [0] * 5 + [1] * 3
        assert out["tok"][b].tolist() == order.tolist() + [0, 1, 2]
        assert torch.isfinite(out["score"][b, :5]).all() and (out["score"][b, 5:] == -INF).all()


@pytest.mark.parametrize("W", [1, 4, 16])
def test_beam_step_all_finished_is_frozen(W):
    """Every beam finished: each keeps its one (w, eos) candidate, so the step only sorts the beams by score (ties
    by slot); scores carry over bit for bit, lengths stay, nothing is live."""
    V, ld, B = 250, 256, 3
    g = torch.Generator().manual_seed(W)
    logits = 3 * torch.randn(B * W, ld, generator=g)
    logits[0, 5] = float("nan")                       # a finished beam's logits are not read
    score = torch.randn(B, W, generator=g) - 3
    if W >= 4:
        score[1, 3] = score[1, 0]                     # an exact tie: slot order
        score[2, 1] = -INF
    length = torch.randint(1, 9, (B, W), generator=g)
    out = run_step(logits, score, torch.ones(B, W, dtype=torch.bool), length, V)
    order = torch.sort(score, dim=1, descending=True, stable=True).indices
    assert torch.equal(out["parent"].long(), order)
    assert torch.equal(out["tok"], torch.full((B, W), EOS))
    assert torch.equal(out["score"], score.gather(1, order))
    assert torch.equal(out["len"].long(), length.gather(1, order))
    assert bool(out["fin"].bool().all()) and out["n_live"] == 0


def test_beam_one_is_greedy_argmax():
    """W = 1 with a zero score: the first index of the row maximum, as asrx_greedy_argmax gives it; a row whose
    logsumexp is NaN (a NaN logit) ties at -inf everywhere and takes index 0 in both."""
    V, ld, B = 250, 256, 8
    logits = 3 * torch.randn(B, ld, generator=torch.Generator().manual_seed(9))
    logits[:, V:] = INF
    logits[1, 40] = logits[1, 7] = logits[1].narrow(0, 0, V).max() + 1      # a tied maximum: the first index
    logits[2, 0] = float("nan")
    logits[3, :V] = float("nan")
    logits[4, :V] = -1.25                                                    # a constant row
    out = run_step(logits, torch.zeros(B, 1), torch.zeros(B, 1, dtype=torch.bool), torch.zeros(B, 1), V)
    lg = logits.to(dev)
    tok, cur = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    K().greedy_argmax(lg, V, tok, cur)
    assert torch.equal(out["tok"].view(B), tok.cpu())
    assert out["tok"].view(B)[1:5].tolist() == [7, 0, 0, 0]
    rows = [0, 5, 6, 7]
    assert torch.equal(out["tok"].view(B)[rows], logits[rows, :V].argmax(dim=1))
    assert torch.equal(out["len"].long().view(B), torch.ones(B, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ gather_rows

def _gather_case(dtype, outer, rows, row_stride, outer_stride, count, offset, index):
    n = outer * outer_stride + offset + 8
    g = torch.Generator().manual_seed(count + offset)
    src_buf = torch.randn(n, generator=g).to(dtype).to(dev)
    dst_buf = torch.full((n,), 512.0, dtype=dtype, device=dev)
    before = dst_buf.clone()
    idx = torch.tensor(index, dtype=torch.int32, device=dev)
    K().gather_rows(src_buf[offset:], dst_buf[offset:], idx, outer, rows, count, row_stride, outer_stride)
    torch.cuda.synchronize()
    expect = before.clone()
    for o in range(outer):
        for r in range(rows):
            if 0 <= index[r] < rows:
                a = offset + o * outer_stride + r * row_stride
                s = offset + o * outer_stride + index[r] * row_stride
                expect[a:a + count] = src_buf[s:s + count]
    assert torch.equal(dst_buf.view(torch.uint8), expect.view(torch.uint8))
    assert not torch.equal(dst_buf, before)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("count", [24, 8, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gather_rows(dtype, count, offset):
    """outer = 2, rows = 6, a permutation with a repeated parent; count = the whole row, an aligned prefix, an
    unaligned prefix; bases on and one element off the 16-byte grid.  Elements beyond count in a row, between the
    rows' extents and around the buffers keep the sentinel."""
    _gather_case(dtype, 2, 6, 24, 6 * 24 + 8, count, offset, [2, 0, 2, 5, 1, 4])


@pytest.mark.parametrize("dtype,count,offset", [(torch.bfloat16, 16384 * 8 + 16, 0), (torch.float32, 2051, 1),
                                                (torch.bfloat16, 70001, 0)])
def test_gather_rows_long_rows(dtype, count, offset):
    """Rows of more than one workgroup's share (the grid-stride loop wraps past 64 blocks of 256 16-byte units) and
    an element-wise row of several blocks; an out-of-range index leaves its row alone."""
    row_stride = (count + 15) // 8 * 8
    _gather_case(dtype, 2, 5, row_stride, 5 * row_stride, count, offset, [4, 4, 0, 7, 1])


def test_gather_rows_cache_layout():
    """The decode loop's call: caches [n][R][P][2d] bf16, the first t + 1 positions of every row moved."""
    n, R, P, d2, t = 3, 8, 9, 64, 4
    g = torch.Generator().manual_seed(1)
    src = torch.randn(n, R, P, d2, generator=g).to(torch.bfloat16).to(dev)
    dst = torch.full_like(src, 512.0)
    index = torch.tensor([0, 0, 2, 1, 5, 5, 5, 4], dtype=torch.int32, device=dev)
    K().gather_rows(src, dst, index, n, R, (t + 1) * d2, P * d2, R * P * d2)
    torch.cuda.synchronize()
    assert torch.equal(dst[:, :, :t + 1], src[:, index.long(), :t + 1])
    assert bool((dst[:, :, t + 1:] == 512.0).all())
