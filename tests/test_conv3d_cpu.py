"""tests/conv3d_ref.py checked on the CPU: its tap loops against F.conv3d / F.conv2d in fp64, the exact family's 2^24 bound and its power to
discriminate on every shape of tests/test_conv3d_gpu.py, the hand-written launch plans against the tiling arithmetic, and the host-only
kernel knob and plan query of csrc/conv3d.hip (no launch, no GPU)."""
import pytest
import torch
import torch.nn.functional as F

import conv3d_ref as R


@pytest.mark.parametrize("N,T,H,W,Cin,Cout", [(2, 3, 5, 7, 8, 12), (1, 1, 4, 3, 5, 4), (3, 4, 2, 1, 3, 6)])
def test_causal_reference_is_conv3d_on_the_causally_padded_input(N, T, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(T * H * W)
    x = torch.randn(N, T, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    r = torch.randn(N, T, H, W, Cout, generator=g, dtype=torch.float64)
    xin = x.permute(0, 4, 1, 2, 3)
    ref = F.conv3d(torch.cat([xin[:, :, :1]] * 2 + [xin], dim=2), w, b, padding=(0, 1, 1)).permute(0, 2, 3, 4, 1)
    assert torch.allclose(R.causal_conv3d_ref(x, w, b), ref, rtol=0, atol=1e-12)
    assert torch.allclose(R.causal_conv3d_ref(x, w, b, r), ref + r, rtol=0, atol=1e-12)
    assert torch.allclose(R.causal_conv3d_ref(x, w), ref - b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("N,T,H,W,Cin,Cout", [(2, 3, 6, 8, 8, 12), (1, 1, 2, 2, 5, 4), (1, 2, 10, 4, 3, 6)])
def test_downsample_reference_is_conv2d_stride_2_on_the_far_edge_padded_input(N, T, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(N, T, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    r = torch.randn(N, T, H // 2, W // 2, Cout, generator=g, dtype=torch.float64)
    xin = x.permute(0, 1, 4, 2, 3).reshape(N * T, Cin, H, W)
    ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w, b, stride=2).reshape(N, T, Cout, H // 2, W // 2).permute(0, 1, 3, 4, 2)
    assert torch.allclose(R.downsample_conv2d_ref(x, w, b), ref, rtol=0, atol=1e-12)
    assert torch.allclose(R.downsample_conv2d_ref(x, w, b, r), ref + r, rtol=0, atol=1e-12)


def test_round_bf16_is_one_round_to_nearest_even():
    # 256..512: bf16 holds even integers; 257 and 259 are ties (-> 256, 260), 1027 lies between 1024 and 1032
    t = torch.tensor([255.0, 257.0, 258.0, 259.0, 261.0, -257.0, 1027.0, 1028.0, 1029.0, 0.0], dtype=torch.float64)
    assert R.round_bf16(t).double().tolist() == [255.0, 256.0, 258.0, 260.0, 260.0, -256.0, 1024.0, 1024.0, 1032.0, 0.0]


@pytest.mark.parametrize("name", list(R.CASES))
def test_exact_family_is_exact_and_discriminates_in_every_tile(name):
    """integers exact in bf16, every partial sum below 2^24 in any order, rounding really happens where a residual is added, and one
    displaced tap (read one pixel to the right; for the single-column shapes, one frame earlier) changes the ROUNDED result in every
    128 x 128 output tile"""
    c = R.CASES[name]
    x, w, bias, res = R.exact_inputs(name)
    for t in (x, w, bias) + (() if res is None else (res,)):
        assert torch.equal(t, t.to(R.BF).float()) and torch.equal(t, t.round())
    assert int(x.abs().max()) == 2 and int(w.abs().max()) == 1
    assert R.exact_bound(name) < R.LIMIT
    ref = R.exact_reference(name)
    assert torch.equal(ref, ref.round())
    want = R.round_bf16(ref)
    if c.res:
        assert int((want.double() != ref).sum()) > 0, "no result of this case needs rounding"
    if c.op == "ds":
        displace = ((0, 0), (0, 1))
    elif c.W == 1:
        displace = ((2, 1, 1), (1, 1, 1))
    else:
        displace = ((2, 1, 1), (2, 1, 2))
    wrong = R.round_bf16(R.reference_of(c, x, w, bias, res, displace))
    a, b = want.view(-1, c.Cout), wrong.view(-1, c.Cout)
    for rows, cols in R.output_tiles(c):
        assert int((a[rows, cols] != b[rows, cols]).sum()) > 0, f"tile {rows} x {cols} does not see the displaced tap"


def _tiling(c):
    M = R.positions(c)
    nbn = -(-c.Cout // 128)
    return M, -(-M // 256) * nbn, -(-M // 128) * nbn


@pytest.mark.parametrize("name", R.PC_CASES)
def test_written_plans_follow_the_tiling(name):
    """the hand-written plans agree with: 256 x 128 tiles, a grid of min(slots, tiles rounded up to 8), slot s walking s, s + grid, ..."""
    c = R.CASES[name]
    M, tiles_pc, tiles_cl = _tiling(c)
    slots = c.slots or 256
    grid = slots if tiles_pc >= slots else -(-tiles_pc // 8) * 8
    assert c.pc == (grid, tiles_pc, -(-tiles_pc // grid)) and c.cl == tiles_cl
    assert c.Cin % 64 == 0 and c.Cout % 4 == 0 and all(p % 4 == 0 for p in c.pads) and c.pads[0] % 8 == 0


def test_case_list_covers_what_it_claims():
    C = R.CASES
    pc = [C[n] for n in R.PC_CASES]
    assert {R.positions(C[n]) for n in ("rows_256", "rows_257", "rows_511")} == {256, 257, 511}
    assert {c.Cout for c in pc} >= {64, 132, 256, 320} and {c.Cin for c in pc} >= {64, 128}
    assert any(c.T == 1 for c in pc) and any(R.out_hw(c)[1] < 4 for c in pc)
    # a tile that straddles samples: 256 rows do not divide into samples
    assert R.positions(C["straddle_64_64"]) < 256 and C["straddle_64_64"].N == 2
    # workgroups that return at once, and workgroups that walk different numbers of tiles, under both epilogues and column-tile counts
    assert any(c.pc[1] < c.pc[0] for c in pc)
    multi = [c for c in pc if c.pc[2] > 1 and c.pc[1] % c.pc[0]]
    assert {(-(-c.Cout // 128), c.res) for c in multi if c.op == "c3" and c.slots == 8} >= {(2, False), (2, True), (3, False), (3, True)}
    assert any(c.slots == 0 and c.pc[2] > 1 for c in multi)
    assert {c.res for c in multi if c.op == "ds"} == {False, True}
    assert any(c.pads != (0, 0, 0) and c.pc[2] > 1 for c in pc)
    assert {(c.Cin, c.Cout) for c in pc if c.op == "c3"} >= R.REAL_PC_PAIRS
    assert {(r[4], r[5]) for r in R.REAL_CONVS if r[8] == 2} == R.REAL_PC_PAIRS


def test_set_kernel_and_plan_on_the_host():
    """vt_conv3d_set_kernel validates and changes nothing on an error; vt_conv3d_plan launches nothing (this runs without a GPU, where the
    device's own slot count falls back to 8) and reports what the forced mode implies"""
    from vt355 import ops
    geo = (2, 4, 16, 19, 64, 256)                        # handover_nbn2: 2432 positions
    try:
        ops.conv3d_set_kernel(2, 8)
        assert ops.conv3d_plan(*geo) == (2, 8, 20, 3)
        for bad in ((3, 0), (-1, 0), (1, 4), (1, 12), (1, -8), (0, 1 << 20)):
            with pytest.raises(RuntimeError):
                ops.conv3d_set_kernel(*bad)
            assert ops.conv3d_plan(*geo) == (2, 8, 20, 3)
        assert ops.conv3d_plan(1, 4, 32, 40, 128, 256, kt=1, stride=2) == (2, 8, 10, 2)
        assert ops.conv3d_plan(2, 3, 5, 7, 64, 132, ldx=72) == (2, 8, 2, 1)
        ops.conv3d_set_kernel(1, 0)
        assert ops.conv3d_plan(*geo) == (1, 38, 38, 1)
        for c in (R.CASES[n] for n in R.PC_CASES):
            kt, stride = (1, 2) if c.op == "ds" else (3, 1)
            assert ops.conv3d_plan(c.N, c.T, c.H, c.W, c.Cin, c.Cout, kt, stride, c.Cin + c.pads[0]) == (1, c.cl, c.cl, 1)
        ops.conv3d_set_kernel(0, 0)
        assert ops.conv3d_plan(*geo)[0] == 1             # one column tile pair, 20 tiles: far below 16 rounds of any grid
        for args in ((2, 4, 16, 19, 60, 256), (2, 4, 16, 19, 64, 254), (0, 4, 16, 19, 64, 256)):
            with pytest.raises(RuntimeError):
                ops.conv3d_plan(*args)
        with pytest.raises(RuntimeError):
            ops.conv3d_plan(*geo, kt=3, stride=2)
        with pytest.raises(RuntimeError):
            ops.conv3d_plan(1, 4, 31, 40, 128, 256, kt=1, stride=2)
    finally:
        ops.conv3d_set_kernel(0, 0)
