"""The eight-phase K-loop of the 256x256 GEMM kernel (gemm_big_bf16.hip, vt_gemm_set_big_loop(2)), bit for bit.

Every case runs three times into poisoned, guarded buffers: under the 128x128 kernel (tile mode 1, held to float64 by
test_gemm_production_gpu.py), under the 256x256 kernel with the two-phase loop (big loop 1) and with the eight-phase loop (big loop 2).
The three buffers -- second outputs and guard rows / columns included -- must hold the same bits: the kernels sum the same MFMA products
in the same K order.  The shapes are the smallest at which the loop's bookkeeping can go wrong: every K-tile count that takes another
path through the prologue / steady pairs / single steady K-tile / last two K-tiles (nk = 1 .. 5) and the odd production count 31, row
and column tiles that are mostly out of range, more output tiles than persistent slots (the cross-tile prefetch, with one K-tile per
output tile and with three), every epilogue, K-extension views, and repeated launches over an LDS that held other bytes."""
import pytest
import torch

from parity import poisoned

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD_ROWS = 3
RM, RN = 300, 260          # two row tiles and two column tiles, the second of each 44 rows / 4 columns wide


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same(x, y):
    return bool(torch.equal(_bits(x), _bits(y)))


def _rand(shape, dev, g, scale=1.0):
    return ((torch.rand(shape, generator=g, device=dev) * 2.0 - 1.0) * scale).to(BF)


class Case:
    """operands of one vt_gemm_bf16 call; run() launches it into fresh poisoned buffers and returns them whole"""

    def __init__(self, dev, M, N, K, *, seed, epi="bias", bias=True, f32=False, pad=0, c_col=0, gates=None, r_mod=0):
        from vt355 import ops
        g = torch.Generator(device=dev).manual_seed(seed)
        self.M, self.N, self.K, self.f32, self.c_col, self.ldc = M, N, K, f32, c_col, N + pad
        self.A = _rand((M, K + pad), dev, g)
        self.W = _rand((N, K + pad), dev, g, K ** -0.5)
        self.a, self.w = self.A[:, :K], self.W[:, :K]
        self.bias = _rand((N,), dev, g, 0.5) if bias else None
        self.epi = {"bias": ops.EPI_BIAS, "gelu": ops.EPI_BIAS_GELU, "gated": ops.EPI_GATED_RES, "dgelu": ops.EPI_DGELU}[epi]
        self.c2 = epi in ("gelu", "gated")
        self.kw = {}
        if epi == "gated":
            self.kw = dict(residual=_rand((r_mod or M, N), dev, g), r_mod=r_mod)
            if gates:
                B, S, St = gates
                tab = torch.rand(B, 2 * N, generator=g, device=dev) + 0.5 + torch.arange(B, device=dev, dtype=torch.float32)[:, None]
                self.kw.update(gate_txt=tab[:, :N], gate_vid=tab[:, N:], gate_bstride=2 * N, S=S, St=St)
                self.tab = tab
        elif epi == "dgelu":
            self.kw = dict(pre_act_in=_rand((M, N), dev, g, 3.0))

    def run(self):
        from vt355 import ops
        dev = self.A.device
        Cb = poisoned((self.M + GUARD_ROWS, self.ldc), torch.float32 if self.f32 else BF, dev)
        C2b = poisoned((self.M + GUARD_ROWS, self.N), BF, dev) if self.c2 else None
        kw = dict(self.kw)
        if self.c2:
            kw["pre_act_out"] = C2b[:self.M]
        ops.gemm(self.a, self.w, Cb[:self.M, self.c_col:self.c_col + self.N], self.bias, epilogue=self.epi, K=self.K, N=self.N, **kw)
        return Cb, C2b


def _modes(tile, loop):
    from vt355 import ops
    ops.gemm_set_tile(tile)
    ops.gemm_set_big_loop(loop)


def _three_ways(case, what):
    """128x128 kernel, 256x256 two-phase, 256x256 eight-phase: the same bits everywhere, guards included"""
    from vt355 import ops
    try:
        _modes(1, 0)
        ref, ref2 = case.run()
        _modes(2, 1)
        assert ops.gemm_kernel(case.M, case.N, case.K) == 2
        two, two2 = case.run()
        _modes(2, 2)
        new, new2 = case.run()
        torch.cuda.synchronize()
    finally:
        _modes(0, 0)
    body = ref[:case.M, case.c_col:case.c_col + case.N]
    assert not bool(torch.isnan(body.float()).any()), f"{what}: the 128x128 reference left poison in the output"
    assert _same(two, ref), f"{what}: two-phase loop differs from the 128x128 kernel"
    assert _same(new, ref), f"{what}: eight-phase loop differs from the 128x128 kernel"
    assert _same(new, two), f"{what}: eight-phase loop differs from the two-phase loop"
    if case.c2:
        assert _same(two2, ref2) and _same(new2, ref2), f"{what}: second output differs"


NKS = [1, 2, 3, 4, 5, 31]


@pytest.mark.parametrize("nk", NKS)
def test_k_tile_counts(dev, nk):
    _three_ways(Case(dev, RM, RN, 64 * nk, seed=100 + nk), f"nk = {nk}")


@pytest.mark.parametrize("K", [64, 192])
def test_generations_and_cross_tile_prefetch(dev, K):
    """17 x 16 + 16 = 288 output tiles on at most 256 slots: some workgroups run two generations, the first K-tile of the second fetched
    under the last K-tile of the first (K = 64: under its only K-tile)"""
    _three_ways(Case(dev, 256 * 17 + 5, 256 * 16, K, seed=200 + K), f"288 tiles, K = {K}")


EPILOGUES = {
    "bias": dict(),
    "no_bias": dict(bias=False),
    "fp32": dict(f32=True),
    "gelu": dict(epi="gelu"),
    "gated_rows": dict(epi="gated", gates=(2, 150, 20), r_mod=150),      # samples shorter than a tile: per-row gate lookup, positional residual
    "gated_tile": dict(epi="gated", gates=(1, 300, 40)),                 # a sample spans the tile: hoisted gates
    "gated_plain": dict(epi="gated", bias=False),                        # residual add without gates
    "dgelu": dict(epi="dgelu", bias=False),
}


@pytest.mark.parametrize("nk", [3, 4])
@pytest.mark.parametrize("name", list(EPILOGUES))
def test_every_epilogue(dev, name, nk):
    _three_ways(Case(dev, RM, RN, 64 * nk, seed=300 + nk, **EPILOGUES[name]), f"{name}, nk = {nk}")


@pytest.mark.parametrize("nk", [3, 4, 31])
def test_strided_operands(dev, nk):
    """the K-extension views: lda = ldw = K + 64, the output a column slice [32, 32 + N) of rows N + 64 wide"""
    _three_ways(Case(dev, RM, RN, 64 * nk, seed=400 + nk, pad=64, c_col=32), f"strided, nk = {nk}")
    _three_ways(Case(dev, RM, RN, 64 * nk, seed=450 + nk, pad=64, c_col=32, epi="gelu"), f"strided gelu, nk = {nk}")


@pytest.mark.parametrize("nk", NKS)
def test_stale_stage_screen(dev, nk):
    """20 launches in a row with a GEMM of another shape through the same kernel in between, so that both LDS stages hold other bytes
    when a launch starts: every output equals the first, guards included.  A fragment read that is placed ahead of the wait that
    retires its stage reads those other bytes whenever the transfer is late -- a sporadic wrong tile, hence 20 launches and not 2."""
    case = Case(dev, RM, RN, 64 * nk, seed=500 + nk)
    other = Case(dev, 700, 520, 128 if nk != 2 else 192, seed=600 + nk)
    try:
        _modes(1, 0)
        ref, _ = case.run()
        _modes(2, 2)
        differs = torch.zeros((), dtype=torch.bool, device=dev)
        for _ in range(20):
            out, _ = case.run()
            differs |= (_bits(out) != _bits(ref)).any()
            other.run()
        torch.cuda.synchronize()
    finally:
        _modes(0, 0)
    assert not bool(differs), f"nk = {nk}: a launch of the eight-phase loop differed from the 128x128 kernel's output"


def test_bad_shapes_are_refused_without_a_launch(dev):
    from vt355 import ops
    from vt355._lib import VtError
    g = torch.Generator(device=dev).manual_seed(7)
    a, w = _rand((RM, 256), dev, g), _rand((RN, 256), dev, g)
    out = poisoned((RM, RN), BF, dev)
    keep = out.clone()
    try:
        _modes(2, 2)
        # VT_ERR_BAD_SHAPE = -1, VT_ERR_BAD_ALIGN = -2 (include/vt355.h): the codes the 128x128 and two-phase paths return
        with pytest.raises(VtError, match=r"vt_gemm_bf16 failed: .*\(code -1\)"):      # K not a multiple of the 64-deep K-tile
            ops.gemm(a, w, out, None, K=100)
        with pytest.raises(VtError, match=r"vt_gemm_bf16 failed: .*\(code -2\)"):      # operand not 16-byte aligned
            ops.gemm(a.view(-1)[4:4 + (RM - 1) * 256].view(RM - 1, 256), w, out[:RM - 1], None)
        with pytest.raises(VtError, match=r"vt_gemm_bf16 failed: .*\(code -2\)"):      # output not 16-byte aligned
            ops.gemm(a, w[:RN - 4], out[:, 2:2 + RN - 4], None)
        with pytest.raises(VtError, match=r"vt_gemm_set_big_loop failed: .*\(code -1\)"):
            ops.gemm_set_big_loop(3)
        torch.cuda.synchronize()
    finally:
        _modes(0, 0)
    assert _same(out, keep), "a refused call wrote to its output"


def test_default_choice_is_one_of_the_two_loops(dev):
    """big loop 0 (the default) picks per shape between two loops that give the same bits: a production shape of each K parity under the
    default equals the forced two-phase loop"""
    from vt355 import ops
    for nk in (30, 31):
        case = Case(dev, 256 * 9 + 77, 1984, 64 * nk, seed=700 + nk)
        try:
            _modes(2, 1)
            two, _ = case.run()
            _modes(2, 0)
            dflt, _ = case.run()
            torch.cuda.synchronize()
        finally:
            _modes(0, 0)
        assert _same(dflt, two), f"default loop choice, nk = {nk}"
