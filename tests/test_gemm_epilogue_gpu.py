"""The epilogue data movement of the 256x256 GEMM kernel (gemm_big_bf16.hip) and the tile argument of ops.gemm, bit for bit.

Every case is launched on the 128x128 kernel (gemm_set_tile(1), held to float64 by test_gemm_production_gpu.py) and on the 256x256 kernel
(gemm_set_tile(2)) under both K-loops, into poisoned buffers that are compared whole -- padding columns, the elements in front of an
offset base pointer and the guard rows behind the matrix included: torch.equal on C and on C2, no tolerance, nothing excluded.
The 256x256 kernel moves C / C2 / R / U 16 bytes at a time where every one of them is 16-byte aligned with ld % 8 == 0 and N % 8 == 0,
and 8 bytes at a time otherwise; ops.gemm_big_last_wide() says which path a launch took, and every case asserts the one it expects.
Shapes: M = 301 (a ragged second row tile of 45 rows, not a multiple of 8 or 16), N = 328 (a second column tile 72 wide; 328 % 8 == 0,
so the aligned cases are wide) and N = 324 (N % 8 == 4: the last 8-column group half valid, always the 8-byte path); K = 64 (one
K-tile) and 512; each of ldc / ldc2 / ldr / ldu once with ld % 8 == 4 and once behind a base pointer offset by 8 bytes."""
import pytest
import torch

from parity import poisoned

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 3 * 332            # elements behind every matrix: three rows of the widest leading dimension
M0, N0 = 301, 328


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same(x, y):
    return bool(torch.equal(_bits(x), _bits(y)))


def _rand(shape, dev, g, scale=1.0):
    return ((torch.rand(shape, generator=g, device=dev) * 2.0 - 1.0) * scale).to(BF)


def _place(flat, M, N, how):
    """an [M, N] view into the flat buffer: 'aligned' ld = N at the base, 'ld4' ld = N + 4 (ld % 8 == 4 for N % 8 == 0), 'ptr8' the base 8
    bytes further (4 bf16)"""
    ld, off = (N + 4, 0) if how == "ld4" else (N, 4) if how == "ptr8" else (N, 0)
    return flat[off:off + M * ld].view(M, ld)[:, :N]


def _flat(M, N, dtype, dev):
    return poisoned((M * (N + 4) + 4 + GUARD,), dtype, dev)


class Case:
    """operands of one ops.gemm call; `where` places one matrix of the epilogue ('C', 'C2', 'R', 'U') off the 16-byte grid"""

    def __init__(self, dev, M, N, K, *, seed, epi="bias", f32=False, where=None, how="aligned", gates=None, r_mod=0, c2=True):
        from vt355 import ops
        g = torch.Generator(device=dev).manual_seed(seed)
        self.M, self.N, self.K, self.f32, self.dev = M, N, K, f32, dev
        self.how = {k: (how if where == k else "aligned") for k in ("C", "C2", "R", "U")}
        self.a, self.w = _rand((M, K), dev, g), _rand((N, K), dev, g, K ** -0.5)
        self.bias = _rand((N,), dev, g, 0.5) if epi != "dgelu" else None
        self.epi = {"bias": ops.EPI_BIAS, "gelu": ops.EPI_BIAS_GELU, "gated": ops.EPI_GATED_RES, "dgelu": ops.EPI_DGELU}[epi]
        self.c2 = epi == "gelu" or (epi == "gated" and c2)
        self.kw = {}
        if epi == "gated":
            rows = r_mod or M
            rflat = torch.zeros(rows * (N + 4) + 4, dtype=BF, device=dev)
            r = _place(rflat, rows, N, self.how["R"])
            r.copy_(_rand((rows, N), dev, g))
            self.kw = dict(residual=r, r_mod=r_mod)
            if gates:
                B, S, St = gates
                tab = torch.rand(B, 2 * N, generator=g, device=dev) + 0.5 + torch.arange(B, device=dev, dtype=torch.float32)[:, None]
                self.kw.update(gate_txt=tab[:, :N], gate_vid=tab[:, N:], gate_bstride=2 * N, S=S, St=St)
        elif epi == "dgelu":
            uflat = torch.zeros(M * (N + 4) + 4, dtype=BF, device=dev)
            u = _place(uflat, M, N, self.how["U"])
            u.copy_(_rand((M, N), dev, g, 3.0))
            self.kw = dict(pre_act_in=u)
        self.wide = where is None and N % 8 == 0

    def run(self):
        from vt355 import ops
        Cb = _flat(self.M, self.N, torch.float32 if self.f32 else BF, self.dev)
        C2b = _flat(self.M, self.N, BF, self.dev) if self.c2 else None
        kw = dict(self.kw)
        if self.c2:
            kw["pre_act_out"] = _place(C2b, self.M, self.N, self.how["C2"])
        ops.gemm(self.a, self.w, _place(Cb, self.M, self.N, self.how["C"]), self.bias, epilogue=self.epi, **kw)
        return Cb, C2b


def _modes(tile, loop):
    from vt355 import ops
    ops.gemm_set_tile(tile)
    ops.gemm_set_big_loop(loop)


def _both_kernels(case, what):
    """the 128x128 kernel once, then the 256x256 kernel under both K-loops: the same bits, and the epilogue path the case expects"""
    from vt355 import ops
    try:
        _modes(1, 0)
        ref, ref2 = case.run()
        got = {}
        for loop in (1, 2):
            _modes(2, loop)
            assert ops.gemm_kernel(case.M, case.N, case.K) == 2
            got[loop] = case.run() + (ops.gemm_big_last_wide(),)
        torch.cuda.synchronize()
    finally:
        _modes(0, 0)
    body = ref[:case.M * case.N] if all(v == "aligned" for v in case.how.values()) else None
    if body is not None:
        assert not bool(torch.isnan(body.float()).any()), f"{what}: the 128x128 reference left poison in the output"
    for loop, (c, c2, wide) in got.items():
        assert wide == int(case.wide), f"{what}, loop {loop}: epilogue path {wide}, expected {int(case.wide)}"
        assert _same(c, ref), f"{what}, loop {loop}: C differs from the 128x128 kernel"
        if case.c2:
            assert _same(c2, ref2), f"{what}, loop {loop}: C2 differs from the 128x128 kernel"


# epilogue -> the matrix placed off the grid; every one of ldc, ldc2, ldr, ldu once with ld % 8 == 4 and once behind an offset base pointer
OFF_GRID = [("bias", "C"), ("gelu", "C2"), ("gated", "R"), ("dgelu", "U")]
GATES = (1, M0, 40)        # one sample spans both row tiles: the hoisted gates


def _kw(epi):
    return dict(epi=epi, gates=GATES) if epi == "gated" else dict(epi=epi)


@pytest.mark.parametrize("K", [64, 512])
@pytest.mark.parametrize("epi", ["bias", "fp32", "gelu", "gated", "dgelu"])
def test_aligned_operands_take_the_wide_path(dev, epi, K):
    kw = dict(f32=True) if epi == "fp32" else _kw(epi)
    _both_kernels(Case(dev, M0, N0, K, seed=1000 + K, **kw), f"{epi}, K = {K}, aligned")


@pytest.mark.parametrize("K", [64, 512])
@pytest.mark.parametrize("how", ["ld4", "ptr8"])
@pytest.mark.parametrize("epi,where", OFF_GRID)
def test_unaligned_operand_takes_the_fallback(dev, epi, where, how, K):
    case = Case(dev, M0, N0, K, seed=2000 + K, where=where, how=how, **_kw(epi))
    assert not case.wide
    _both_kernels(case, f"{epi}, K = {K}, {where} {how}")


@pytest.mark.parametrize("K", [64, 512])
@pytest.mark.parametrize("epi", ["bias", "fp32", "gelu", "gated", "dgelu"])
def test_half_valid_last_column_group(dev, epi, K):
    """N = 324: N % 8 == 4, the 8-byte path for the whole launch"""
    kw = dict(f32=True) if epi == "fp32" else _kw(epi)
    case = Case(dev, M0, 324, K, seed=3000 + K, **kw)
    assert not case.wide
    _both_kernels(case, f"{epi}, K = {K}, N = 324")


@pytest.mark.parametrize("K", [64, 512])
def test_gated_sample_and_text_boundaries_inside_a_tile(dev, K):
    """B = 3, S = 130, St = 7: a 256-row tile holds a sample boundary and text / video boundaries (per-row gate lookup); the residual a
    positional table of 130 rows; without the second output as well; and the same rows with fp32 output under the bias epilogue"""
    _both_kernels(Case(dev, 390, N0, K, seed=4000 + K, epi="gated", gates=(3, 130, 7), r_mod=130), f"gated r_mod, K = {K}")
    _both_kernels(Case(dev, 390, N0, K, seed=4100 + K, epi="gated", gates=(3, 130, 7), r_mod=130, c2=False), f"gated r_mod no C2, K = {K}")
    _both_kernels(Case(dev, 390, N0, K, seed=4200 + K, f32=True), f"fp32 bias, M = 390, K = {K}")


def test_second_generation_reuses_the_slab(dev):
    """4160 x 4096: 17 x 16 = 272 output tiles, so on 256 slots 16 workgroups run a second tile through the cross-tile prefetch and the
    slab the first one left"""
    _both_kernels(Case(dev, 4160, 4096, 128, seed=5000), "272 tiles")
    _both_kernels(Case(dev, 4160, 4096, 128, seed=5001, epi="dgelu"), "272 tiles, dgelu")


def test_tile_argument(dev):
    """ops.gemm(..., tile=2 / 3) against tile=0: equal results; tile=2 reaches the 256x256 kernel (seen through its epilogue path word),
    a global gemm_set_tile mode wins over the argument, a tile outside 0..3 is refused"""
    from vt355 import ops
    from vt355._lib import VtError
    M, N, K = 600, 1920, 256
    g = torch.Generator(device=dev).manual_seed(6000)
    a, w, bias = _rand((M, K), dev, g), _rand((N, K), dev, g, K ** -0.5), _rand((N,), dev, g, 0.5)
    assert ops.gemm_kernel(M, N, K) == 1           # the shape rule leaves this on the 128x128 kernel
    outs = {}
    try:
        off = poisoned((M, N + 4), BF, dev)
        ops.gemm(a, w, off[:, :N], bias, tile=2)   # ld % 8 == 4: the path word goes to 0
        assert ops.gemm_big_last_wide() == 0
        outs[0] = ops.gemm(a, w, poisoned((M, N), BF, dev), bias, tile=0)
        assert ops.gemm_big_last_wide() == 0       # not the 256x256 kernel
        outs[3] = ops.gemm(a, w, poisoned((M, N), BF, dev), bias, tile=3)
        assert ops.gemm_big_last_wide() == 0
        outs[2] = ops.gemm(a, w, poisoned((M, N), BF, dev), bias, tile=2)
        assert ops.gemm_big_last_wide() == 1       # the 256x256 kernel, aligned
        ops.gemm(a, w, off[:, :N], bias, tile=2)
        ops.gemm_set_tile(1)
        outs["mode 1"] = ops.gemm(a, w, poisoned((M, N), BF, dev), bias, tile=2)
        assert ops.gemm_big_last_wide() == 0       # the global mode won: no 256x256 launch
        ops.gemm_set_tile(0)
        with pytest.raises(VtError, match=r"vt_gemm_bf16 failed: .*\(code -1\)"):
            ops.gemm(a, w, poisoned((M, N), BF, dev), bias, tile=4)
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_tile(0)
    assert not bool(torch.isnan(outs[0].float()).any())
    assert _same(off[:, :N], outs[0])
    for k in (2, 3, "mode 1"):
        assert _same(outs[k], outs[0]), f"tile = {k} differs from tile = 0"


def test_dispatch_answers(dev):
    from vt355 import ops
    assert ops.gemm_kernel(71104, 1920, 7680) == 3           # the shape rule is where it was
    assert ops.gemm_block_tile(71104, 1920, 7680) == 2
    assert ops.gemm_block_tile(71104, 1984, 7744) == 2
    assert ops.gemm_block_tile(71104, 1152, 7680) == 0
    assert ops.gemm_block_tile(512, 1920, 7680) == 0
