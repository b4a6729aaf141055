"""Column sums (csrc/norm.hip: asrx_reduce_rows, asrx_reduce_rows_grouped) bit for bit on integer inputs.

Inputs are integers in [-4, 4] (exact in bf16 and fp32), so every order of addition gives the same fp32 sum and
`out` must equal it exactly: no tolerance.  Row counts sit on both sides of the grouped kernel's 64-row trips and
4-row slices (59..65, 124..128), of the two-stage kernel's rows-per-block split (nblocks 1, 3, 512, more blocks
than rows included) and at 0; column counts on both sides of the 64-column chunk.  `out` and the partials lie
between sentinels that must not change.  On the MI355X with the kernels of commit ef27a9a all 15 cases (720 two-stage
launches, 64- and 65-group tables) were exact on their first run."""
import pytest
import torch

import rowkernel_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, B16 = R.F32, R.B16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import asrx
    asrx.native()


def K():
    from asrx import kernels
    return kernels


def _diff(got, want, what):
    ne = (got != want).nonzero().reshape(-1)
    return f"{what}: {ne.numel()} of {got.numel()} columns differ, first {int(ne[0]) if ne.numel() else -1}"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nblocks", R.RR_NBLOCKS)
@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_reduce_rows_exact(dtype, nblocks, accumulate):
    k = K()
    for rows in R.RR_ROWS:
        for cols in R.RR_COLS:
            ld = cols + 3
            x = R.int_rows(max(rows, 1), ld, 4, rows * 131 + cols, dtype)
            init = R.int_rows(1, cols, 4, cols, F32)[0]
            obuf, out = R.guarded(cols, F32, dev)
            out.copy_(init)
            pbuf, part = R.guarded(nblocks * cols, F32, dev)
            xd = x.to(dev)
            k.call("asrx_reduce_rows", k.code(x), xd.data_ptr(), rows, cols, ld, out.data_ptr(), accumulate,
                   part.data_ptr(), nblocks, k.stream())
            torch.cuda.synchronize()
            want = x[:rows, :cols].double().sum(0).to(F32) + (init if accumulate else 0)
            what = f"rows {rows} cols {cols}"
            assert R.same_bits(out.cpu(), want), _diff(out.cpu(), want, what)
            assert R.guards_intact(obuf, cols) and R.guards_intact(pbuf, nblocks * cols), what


def _groups(count, with_empty):
    """count groups over R.RR_ROWS x R.RR_COLS: (device input [rows, cols], host input, init, guarded out)"""
    rows_of = [r for r in R.RR_ROWS if with_empty or r > 0]
    groups = []
    for i in range(count):
        rows, cols = rows_of[i % len(rows_of)], R.RR_COLS[(i // len(rows_of) + i) % len(R.RR_COLS)]
        x = R.int_rows(max(rows, 1), cols, 4, i, F32)
        init = R.int_rows(1, cols, 4, 500 + i, F32)[0]
        obuf, out = R.guarded(cols, F32, dev)
        out.copy_(init)
        groups.append((x.to(dev), x, rows, cols, init, obuf, out, i % 3 != 0))
    return groups


def _check_groups(groups):
    torch.cuda.synchronize()
    for i, (_, x, rows, cols, init, obuf, out, acc) in enumerate(groups):
        want = x[:rows].double().sum(0).to(F32) + (init if acc else 0)
        what = f"group {i} rows {rows} cols {cols} accumulate {acc}"
        assert R.same_bits(out.cpu(), want), _diff(out.cpu(), want, what)
        assert R.guards_intact(obuf, cols), what


@pytest.mark.parametrize("count", R.RR_GROUPS)
def test_reduce_rows_grouped_exact(count):
    """kernels.reduce_rows_grouped on 64 groups (one launch, the table full) and 65 (the wrapper's split)"""
    assert K().MAX_ROWSUM_GROUPS == R.RG_MAX
    groups = _groups(count, with_empty=False)
    K().reduce_rows_grouped([(xd[:rows], out, acc) for xd, _, rows, _, _, _, out, acc in groups])
    _check_groups(groups)


def test_reduce_rows_grouped_table_limits():
    """The C ABI itself: a full table with empty groups (rows = 0: out = 0, or unchanged when accumulating), and a
    table of RG_MAX + 1 refused with nothing written."""
    k = K()

    def table(groups):
        arr = (k.RowsumGroup * len(groups))()
        for gr, (xd, _, rows, cols, _, _, out, acc) in zip(arr, groups):
            gr.in_, gr.rows, gr.cols, gr.out, gr.accumulate = xd.data_ptr(), rows, cols, out.data_ptr(), int(acc)
        return arr
    groups = _groups(R.RG_MAX, with_empty=True)
    assert sum(1 for g in groups if g[2] == 0) >= 4
    k.call("asrx_reduce_rows_grouped", table(groups), len(groups), k.stream())
    _check_groups(groups)
    groups = _groups(R.RG_MAX + 1, with_empty=True)
    with pytest.raises(RuntimeError, match="bad argument"):
        k.call("asrx_reduce_rows_grouped", table(groups), len(groups), k.stream())
    torch.cuda.synchronize()
    for _, _, _, cols, init, obuf, out, _ in groups:
        assert R.same_bits(out.cpu(), init) and R.guards_intact(obuf, cols)
