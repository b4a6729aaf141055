"""asrx_ctc_align_long on the GPU against tests/ctc_align_ref.py: transcripts of up to 4095 labels, a workgroup of NW =
ceil((Lmax + 1) / 256) waves per sample.

The rules are those of tests/test_gpu_ctc_align_kernels.py: the kernel's path must be a valid alignment whose fp64
score lies within `bound` (4 x the fp32 reference's own error, floored at 1e-5 * max(1, |value|)) of the fp64 optimum;
score, frame_logp and tok_conf lie within the bound of their fp64 values on THAT path; the spans are the run boundaries
of frame_pos exactly; and where a case is marked exact it asserts, on the input, that the reference's on-path margin is
>= 10 x the bound, and then that frame_pos equals the reference's.

The L = 4095 case has no fp64 recursion (its T x S arrays): there the path is pinned by the input alone.  The test
asserts that the planted symbol of every frame beats every other symbol of that frame by >= 10 x the bound; then the
planted path has the largest log-probability at every frame, so it is the unique optimum, and its fp64 / fp32 sums
give the reference score and the fp32 error the bound derives from."""
import functools

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R
from tests.test_gpu_ctc_align_kernels import BLANK, _planted, _rand, bits, labels

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def seam_labels(n, V, seed, at):
    """n labels without adjacent repeats except label[at - 1] == label[at] (pairs in different waves for at % 256 == 0)."""
    out = labels(n, V, seed)
    out[at] = out[at - 1]
    while out[at + 1] == out[at] or out[at + 1] == BLANK or out[at + 1] == out[at + 2]:
        out[at + 1] = (out[at + 1] + 1) % V
    assert sum(a == b for a, b in zip(out, out[1:])) == 1
    return out


def _edge(L, seed):
    """Planted, exact: L and L // 2 labels (the second with repeats), T = L + 40."""
    return dict(T=L + 40, V=250, ld=256, Lmax=L, targets=[labels(L, 250, seed), labels(L // 2, 250, seed + 100, 7)],
                lengths=None, gen="planted", boost=8.0, noise=0.5, seed=seed, exact=True)


CASES = [_edge(L, 100 + k) for k, L in enumerate([255, 256, 257, 511, 512, 767, 1023, 1024, 2047])] + [
    # random logits with a boosted blank up to L = 1100: fp32 may take another path of (nearly) the same score
    dict(T=700, V=250, ld=256, Lmax=300, targets=[labels(300, 250, 30), labels(280, 250, 31, 6)], lengths=None,
         gen="rand", seed=20, exact=False),
    dict(T=2300, V=250, ld=256, Lmax=1100, targets=[labels(1100, 250, 32), labels(513, 250, 33)], lengths=(2300, 1200),
         gen="rand", seed=21, exact=False),
    # equal labels across a seam at the only feasible length (T_b = L + 1) and one frame short; beside them
    # T_b = L without repeats (a single alignment as well)
    dict(T=302, V=20, ld=20, Lmax=301, targets=[seam_labels(301, 20, 40, 256)] * 2 + [labels(9, 20, 41)],
         lengths=(302, 301, 9), gen="rand", seed=22, exact=True),
    dict(T=558, V=257, ld=320, Lmax=557, targets=[seam_labels(557, 257, 42, 512)] * 2 + [labels(9, 257, 43)],
         lengths=(558, 557, 9), gen="rand", seed=23, exact=True),
    # waves without a live pair under a long bound; input lengths (T, short, 0: the empty alignment), V 5 / ld 8
    dict(T=760, V=5, ld=8, Lmax=700, targets=[labels(700, 5, 44), labels(3, 5, 45), [], labels(300, 5, 46, 5)],
         lengths=(760, 40, 0, 500), gen="planted", boost=8.0, noise=0.5, seed=24, exact=True),
    # the same kind of batch under the widest bound (NW = 16), a row stride that is no multiple of 4
    dict(T=330, V=250, ld=251, Lmax=4095, targets=[labels(300, 250, 47), [9]], lengths=None, gen="planted",
         boost=8.0, noise=0.5, seed=25, exact=True),
    # malformed labels beyond the first wave (the blank at position 300, V at 600), a length above the bound, a good one
    dict(T=700, V=250, ld=256, Lmax=650,
         targets=[labels(300, 250, 48) + [BLANK] + labels(349, 250, 49), labels(600, 250, 50) + [250] + labels(49, 250, 51),
                  labels(650, 250, 52), labels(650, 250, 53)], tlens=(650, 650, 651, 650), lengths=None, gen="planted",
         boost=8.0, noise=0.5, seed=26, exact=True),
]
for _c in CASES:
    _c["B"] = len(_c["targets"])


@functools.lru_cache(maxsize=None)
def case(i):
    """tests/test_gpu_ctc_align_kernels.py's case(): inputs, per-sample fp64 references and the fp32 reference's error,
    computed once and never changed."""
    c = CASES[i]
    x = _rand(c) if c["gen"] == "rand" else _planted(c)
    W = max(c["Lmax"], max(len(t) for t in c["targets"]), 1)
    tg = torch.full((c["B"], W), BLANK, dtype=torch.int64)
    for b, t in enumerate(c["targets"]):
        tg[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
    tl = torch.tensor(c.get("tlens", [len(t) for t in c["targets"]]), dtype=torch.int32)
    refs, errs = [], []
    for b in range(c["B"]):
        L = int(tl[b])
        Tb = c["T"] if c["lengths"] is None else c["lengths"][b]
        if L < 0 or L > c["Lmax"]:
            refs.append(R.no_alignment(c["T"], c["Lmax"]))
            errs.append(0.0)
            continue
        xb = x[b, :, :c["V"]].numpy()
        r64 = R.viterbi(xb, c["targets"][b][:L], BLANK, Tb, c["Lmax"])
        r32 = R.viterbi(xb, c["targets"][b][:L], BLANK, Tb, c["Lmax"], dtype=np.float32)
        refs.append(r64)
        errs.append(abs(r64["score"] - r32["score"]) if r64["feasible"] else 0.0)
    return c, x, tg, tl, refs, errs


GARBAGE_I, GARBAGE_F = 0x7f7f7f7f, float("nan")


def launch(c, x, tg, tl):
    """The C entry point on buffers filled with garbage: every element of every output must be written."""
    from asrx._lib import call
    from asrx import kernels as K
    B, T, ld, Lmax = c["B"], c["T"], c["ld"], c["Lmax"]
    xd = x.reshape(B * T, ld).to(dev)
    tgd, tld = tg.to(dev), tl.to(dev)
    il = None if c["lengths"] is None else torch.tensor(c["lengths"], dtype=torch.int32, device=dev)
    words = K.ctc_align_workspace_words(B, T, Lmax, long=True)
    ws = torch.full((words,), GARBAGE_I, dtype=torch.int32, device=dev)
    fp = torch.full((B, T), GARBAGE_I, dtype=torch.int32, device=dev)
    fl = torch.full((B, T), GARBAGE_F, dtype=torch.float32, device=dev)
    st = torch.full((B, Lmax), GARBAGE_I, dtype=torch.int32, device=dev)
    en = torch.full((B, Lmax), GARBAGE_I, dtype=torch.int32, device=dev)
    cf = torch.full((B, Lmax), GARBAGE_F, dtype=torch.float32, device=dev)
    sc = torch.full((B,), GARBAGE_F, dtype=torch.float32, device=dev)
    call("asrx_ctc_align_long", xd.data_ptr(), B, T, c["V"], ld, tgd.data_ptr(), tgd.stride(0),
         None if il is None else il.data_ptr(), tld.data_ptr(), Lmax, BLANK, ws.data_ptr(), words, fp.data_ptr(),
         fl.data_ptr(), st.data_ptr(), en.data_ptr(), cf.data_ptr(), sc.data_ptr(), K.stream())
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in (fp, fl, st, en, cf, sc))


def check_sample(label, x_b, target, Tb, Lmax, ref_score, err32, got_b, want_pos=None):
    """One feasible sample's outputs against the fp64 quantities on the kernel's own path; returns error / bound."""
    fp, fl, st, en, cf, sc = got_b
    L = len(target)
    bound = R.bound(err32, ref_score)
    pos = fp.numpy()
    assert R.path_is_valid(pos, target, Tb), (label, pos.tolist())
    total, flp = R.rescore(x_b, target, BLANK, pos, Tb)
    assert total >= ref_score - bound and total <= ref_score + 1e-9, (label, total, ref_score)
    err = abs(float(sc) - total)
    assert err <= bound, (label, float(sc), total, bound)
    assert (fl[Tb:] == 0).all()
    flb = np.array([R.bound(err32, v) for v in flp[:Tb]])
    assert (np.abs(fl[:Tb].double().numpy() - flp[:Tb]) <= flb).all(), label
    ws, we, wc = R.spans_of(pos, flp, L, Lmax)
    assert st.tolist() == ws.tolist() and en.tolist() == we.tolist(), label
    cfb = np.array([R.bound(err32, v) for v in wc])
    assert (np.abs(cf.double().numpy() - wc) <= cfb).all(), label
    assert all(we[u] > ws[u] and (u == 0 or ws[u] >= we[u - 1]) for u in range(L)), label
    if want_pos is not None:
        assert pos.tolist() == list(want_pos), label
    return err / bound


@pytest.mark.parametrize("i", range(len(CASES)))
def test_align_long_matches_reference(i):
    c, x, tg, tl, refs, errs = case(i)
    T, Lmax = c["T"], c["Lmax"]
    got = launch(c, x, tg, tl)
    fp, fl, st, en, cf, sc = got
    worst = 0.0
    for b, r in enumerate(refs):
        L = int(tl[b])
        Tb = T if c["lengths"] is None else c["lengths"][b]
        if not r["feasible"]:
            assert float(sc[b]) == -INF, (b, float(sc[b]))
            assert (fp[b] == -1).all() and (fl[b] == 0).all()
            assert (st[b] == -1).all() and (en[b] == -1).all() and (cf[b] == 0).all()
            continue
        bound = R.bound(errs[b], r["score"])
        print(f"long case {i} sample {b}: L {L}, T_b {Tb}, score {r['score']:.4f}, fp32 reference error "
              f"{errs[b]:.2e}, bound {bound:.2e}, on-path margin {r['margin']:.3e} = {r['margin'] / bound:.1f} x bound")
        if c["exact"]:
            assert r["margin"] >= 10 * bound, (b, r["margin"], bound)     # a condition on the input
        worst = max(worst, check_sample((i, b), x[b, :, :c["V"]].numpy(), c["targets"][b][:L], Tb, Lmax, r["score"],
                                        errs[b], tuple(o[b] for o in got),
                                        r["frame_pos"].tolist() if c["exact"] else None))
    print(f"long case {i}: worst score error / bound {worst:.3f}")
    again = launch(c, x, tg, tl)
    for a, b_ in zip(got, again):
        assert torch.equal(bits(a), bits(b_))      # the same inputs give the same bits


def test_cases_cover_the_code_paths():
    exact = [c for c in CASES if c["exact"]]
    assert {1, 2, 3, 4, 5, 8, 16} <= {c["Lmax"] // 256 + 1 for c in exact}
    assert {255, 256, 257, 511, 512, 767, 1023, 1024, 2047} <= {len(t) for c in exact for t in c["targets"]}
    assert {(5, 8), (250, 256), (257, 320)} <= {(c["V"], c["ld"]) for c in CASES} and any(c["ld"] % 4 for c in CASES)
    assert any(not c["exact"] and c["Lmax"] >= 1100 for c in CASES)
    assert any(c["lengths"] and 0 in c["lengths"] for c in CASES)


@functools.lru_cache(maxsize=None)
def longest_case():
    """L = 4095 planted in T = 4200 frames: (case, logits, targets, lengths, planted frame_pos, fp64 score of the
    planted path, fp32 error of that sum, the smallest per-frame margin of the planted symbol)."""
    L, T, V = 4095, 4200, 250
    target = labels(L, V, 60)
    c = dict(B=1, T=T, V=V, ld=256, Lmax=L, targets=[target], lengths=None, gen="planted", boost=8.0, noise=0.5, seed=27)
    x = _planted(c)
    edges = np.linspace(0, T, L + 1).astype(int)         # ctc_align_ref.planted's runs (no adjacent equal labels)
    pos = np.repeat(np.arange(L), np.diff(edges))
    sym = np.asarray(target)[pos]
    lp64 = R.log_softmax(x[0, :, :V].numpy())
    lp32 = R.log_softmax(x[0, :, :V].numpy(), np.float32)
    on = lp64[np.arange(T), sym]
    rest = lp64.copy()
    rest[np.arange(T), sym] = -np.inf
    margin = float((on - rest.max(axis=1)).min())
    s32 = np.float32(0.0)
    for v in lp32[np.arange(T), sym]:
        s32 = np.float32(s32 + v)
    tg = torch.tensor([target], dtype=torch.int64)
    return c, x, tg, torch.tensor([L], dtype=torch.int32), pos, float(on.sum()), abs(float(s32) - float(on.sum())), margin


def test_the_longest_transcript_planted():
    c, x, tg, tl, pos, score, err32, margin = longest_case()
    bound = R.bound(err32, score)
    print(f"long L4095: score {score:.4f}, fp32 error of the sum {err32:.2e}, bound {bound:.2e}, smallest per-frame "
          f"margin {margin:.3f} = {margin / bound:.1f} x bound")
    assert margin >= 10 * bound                     # a condition on the input: the planted path is the unique optimum
    got = launch(c, x, tg, tl)
    ratio = check_sample("L4095", x[0, :, :c["V"]].numpy(), c["targets"][0], c["T"], c["Lmax"], score, err32,
                         tuple(o[0] for o in got), pos.tolist())
    print(f"long L4095: worst score error / bound {ratio:.3f}")


def test_wrapper_and_bit_identical_repeats():
    """kernels.ctc_align(long=True) gives the C call's bits, twice; its default still refuses 256 columns."""
    from asrx import kernels as K
    c, x, tg, tl, _, _ = case(1)
    want = launch(c, x, tg, tl)
    B, T, ld = c["B"], c["T"], c["ld"]
    xd = x.reshape(B * T, ld).to(dev)
    for _ in range(2):
        out = K.ctc_align(xd, c["V"], T, tg.to(dev), tl.to(dev), None, max_target_len=c["Lmax"], blank=BLANK, long=True)
        torch.cuda.synchronize()
        for a, b in zip(out[:6], want):
            assert torch.equal(bits(a.cpu()), bits(b))
    with pytest.raises(RuntimeError, match="unsupported"):
        K.ctc_align(xd, c["V"], T, tg.to(dev), tl.to(dev), None)
    with pytest.raises(RuntimeError, match="unsupported"):
        K.ctc_align(xd, c["V"], T, torch.zeros(B, 4096, dtype=torch.int64, device=dev), tl.to(dev), None, long=True)
