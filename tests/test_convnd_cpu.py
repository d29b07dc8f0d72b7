"""tests/convnd_ref.py checked on the CPU: its tap loops against F.conv3d and autograd in fp64 on every case geometry, the zero-insertion
route of the stride-2 input gradient, the exact family's bounds and its power to discriminate, its order-independence in fp32, the
hand-written launch plans against the host-only plan queries of csrc/convnd.hip (no launch, no GPU: the library then assumes 256 CUs), and
the real UNet's convolution list against vt355.unet.build_structure."""
import pytest
import torch
import torch.nn.functional as F

import convnd_ref as R


def _geometries():
    """the distinct (N, T, H, W, kernel, padding, stride) of the cases.  The tap loops treat channels as a matrix product, so the comparison
    with F.conv3d runs on 6 -> 5 channels whatever the case's own channel counts"""
    seen = {}
    for n, c in R.CASES.items():
        seen.setdefault((c.N, c.T, c.H, c.W, c.k, c.pad, c.stride), n)
    return [pytest.param(*g, id=n) for g, n in seen.items()]


@pytest.mark.parametrize("N,T,H,W,k,pad,stride", _geometries())
def test_tap_loops_are_conv3d_and_its_autograd(N, T, H, W, k, pad, stride):
    """forward (+ bias, per-sample bias, residual), dX (adjoint loop; for stride 1 and for even stride-2 shapes also the route the UNet
    takes), dW in the packed layout and db, against F.conv3d / autograd in fp64: round-off only"""
    Cin, Cout = 6, 5
    g = torch.Generator().manual_seed(N * T + H * W)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w, b = rn(N, T, H, W, Cin).requires_grad_(True), rn(Cout, Cin, *k).requires_grad_(True), rn(Cout).requires_grad_(True)
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, b, stride=(1, stride, stride), padding=pad).permute(0, 2, 3, 4, 1)
    Ho, Wo = R.out_hw(H, W, k, pad, stride)
    assert tuple(y.shape) == (N, T, Ho, Wo, Cout)
    sb, res, dy = rn(N, Cout), rn(*y.shape), rn(*y.shape)
    (y * dy).sum().backward()
    tol = dict(rtol=0, atol=1e-11)
    assert torch.allclose(R.conv_ref(x.detach(), w.detach(), k, pad, stride, b.detach()), y.detach(), **tol)
    assert torch.allclose(R.conv_ref(x.detach(), w.detach(), k, pad, stride), y.detach() - b.detach(), **tol)
    assert torch.allclose(R.conv_ref(x.detach(), w.detach(), k, pad, stride, b.detach(), sb, res), y.detach() + sb[:, None, None, None] + res, **tol)
    assert torch.allclose(R.conv_dx_ref(dy, w.detach(), k, pad, stride, H, W), x.grad, **tol)
    if stride == 1:
        assert torch.allclose(R.conv_ref(dy, R.dx_weight(w.detach()), k, pad, 1), x.grad, **tol)
    elif H == 2 * Ho and W == 2 * Wo:
        assert torch.allclose(R.conv_dx_zero_insert_ref(dy, w.detach(), k, pad), x.grad, **tol)
    dw = w.grad.permute(0, 2, 3, 4, 1).reshape(Cout, -1)                       # [Cout, (dt, dh, dw), Cin]: the packed layout
    assert torch.allclose(R.conv_dw_ref(dy, x.detach(), k, pad, stride), dw, **tol)
    assert torch.allclose(R.conv_db_ref(dy), b.grad, **tol)


def test_packed_layout_is_the_librarys():
    from vt355 import ops
    g = torch.Generator().manual_seed(5)
    w = torch.randn(5, 6, 3, 2, 4, generator=g)
    assert torch.equal(ops.pack_conv_weight_nd(w), w.permute(0, 2, 3, 4, 1).reshape(5, -1))
    assert torch.equal(ops.pack_conv_weight_dx(w), ops.pack_conv_weight_nd(R.dx_weight(w)))


def test_round_bf16_is_one_round_to_nearest_even():
    # 128..256: bf16 holds integers, so .5 is a tie and .25 / .75 round to the nearer; 256..512: even integers only
    t = torch.tensor([130.25, 130.5, 131.5, 131.75, -130.5, 255.0, 257.0, 258.0, 259.0, 260.75, 261.0, 0.25], dtype=torch.float64)
    assert R.round_bf16(t).double().tolist() == [130.0, 130.0, 132.0, 132.0, -130.0, 255.0, 256.0, 258.0, 260.0, 260.0, 260.0, 0.25]


@pytest.mark.parametrize("name", list(R.CASES))
def test_exact_family_keeps_its_rule(name):
    """values exact in bf16 (sbias: multiples of 0.25 in fp32); every partial sum in any order below 2^22 (forward, quarters) / 2^24
    (gradients, integers); with a residual at least a quarter of the outputs lie beyond 256 and are really rounded"""
    c = R.CASES[name]
    d = R.exact_inputs(name)
    for key in ("x", "w", "bias", "res", "dy", "dw_fill", "db_fill"):
        if d[key] is not None:
            assert torch.equal(d[key], d[key].to(R.BF).float()) and torch.equal(d[key], d[key].round()), key
    if d["sbias"] is not None:
        assert torch.equal(4 * d["sbias"], (4 * d["sbias"]).round()) and int((d["sbias"] != d["sbias"].round()).sum()) > 0
    assert int(d["x"].abs().max()) == 2 and int(d["w"].abs().max()) == 1 and int(d["dy"].abs().max()) == 2
    fwd, dx, dw, db = R.exact_bounds(name)
    assert 4 * fwd < R.LIMIT and dx < R.LIMIT and dw < R.LIMIT and db < R.LIMIT, (fwd, dx, dw, db)
    if "f" in c.run:
        ref = R.exact_forward(name)
        assert torch.equal(4 * ref, (4 * ref).round())
        if c.res:
            assert (ref.abs() > 256).double().mean().item() >= 0.25
            assert int((R.round_bf16(ref).double() != ref).sum()) > 0, "no result of this case needs rounding"
    if "w" in c.run:
        dwr, dbr = R.exact_weight_grad(name)
        assert torch.equal(dwr, dwr.round()) and torch.equal(dbr, dbr.round())


# A displaced tap changes its term of every output, sum_ci w (x[elsewhere] - x[there]): 64 or more products of integers in [-2, 2] and
# {-1, 0, 1}, standard deviation >= 13 -- far more than bf16's spacing at these magnitudes (at most 4 below 1024).  The outputs that cannot
# change are those where both reads fall into the zero padding: at most one line or column in `extent` of the displaced axis.  HALF of all
# outputs is a share the true inputs meet on every case with room to spare, and one no convolution with a wrong tap can stay under.
SHARE = 0.5


@pytest.mark.parametrize("name", R.FWD_CASES)
def test_every_displaced_tap_shows_after_rounding(name):
    c = R.CASES[name]
    d = R.exact_inputs(name)
    ref = R.exact_forward(name)
    want = R.round_bf16(ref)
    Ho, Wo = R.case_hw(c)
    xp = R._padded(d["x"].double(), c.pad)
    w = d["w"].double()
    for tap, off in R.displaced(c):
        wt = w[:, :, tap[0], tap[1], tap[2]].t()
        delta = (R._tap_rows(xp, off, c.T, Ho, Wo, c.stride) - R._tap_rows(xp, tap, c.T, Ho, Wo, c.stride)) @ wt
        wrong = R.round_bf16(ref + delta.view(ref.shape))
        share = (wrong != want).double().mean().item()
        assert share >= SHARE, f"tap {tap} read at {off}: only {share:.3f} of the rounded outputs change"
    # the incremental form above is the displaced reference itself
    tap, off = R.displaced(c)[-1]
    assert torch.equal(R.round_bf16(R.forward_of(c, d, (tap, off))), wrong)


@pytest.mark.parametrize("name", R.DW_CASES)
def test_a_dropped_last_row_changes_the_weight_gradient(name):
    c = R.CASES[name]
    d = R.exact_inputs(name)
    full, _ = R.exact_weight_grad(name)
    short = R.conv_dw_ref(d["dy"], d["x"], c.k, c.pad, c.stride, rows=R.positions(c) - 1)
    assert int((full.float() != short.float()).sum()) > 0
    assert int((R.conv_db_ref(d["dy"]).float() != R.conv_db_ref(d["dy"].reshape(-1, c.Cout)[:-1]).float()).sum()) > 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_accumulation_in_a_shuffled_order_is_exact(name):
    """the device-independent claim: fp32 sums of the family equal the fp64 sums whatever the order -- taps and channels shuffled for the
    forward, positions shuffled and cut into uneven splits that are added one after the other (as the atomics do) for the gradients"""
    c = R.CASES[name]
    d = R.exact_inputs(name)
    g = torch.Generator().manual_seed(R._seed(name))
    Ho, Wo = R.case_hw(c)
    xp = R._padded(d["x"].double(), c.pad).float()
    taps = R.taps_of(c.k)
    if "f" in c.run:
        y = torch.zeros(R.positions(c), c.Cout)
        perm = torch.randperm(c.Cin, generator=g)
        for i in torch.randperm(len(taps), generator=g).tolist():
            tap = taps[i]
            rows, wt = R._tap_rows(xp, tap, c.T, Ho, Wo, c.stride), d["w"][:, :, tap[0], tap[1], tap[2]].t()
            for lo in range(0, c.Cin, 32):
                y += rows[:, perm[lo:lo + 32]] @ wt[perm[lo:lo + 32]]
        y = y.view(c.N, c.T, Ho, Wo, c.Cout) + d["bias"]
        if c.sb:
            y = y + d["sbias"][:, None, None, None, :]
        if c.res:
            y = y + d["res"]
        assert y.dtype == torch.float32 and torch.equal(y.double(), R.exact_forward(name))
    if "w" in c.run:
        M = R.positions(c)
        order = torch.randperm(M, generator=g)
        dy2 = d["dy"].reshape(M, c.Cout)[order]
        cuts = sorted(set([0, M] + torch.randint(0, M, (4,), generator=g).tolist()))
        dw, db = d["dw_fill"].clone(), d["db_fill"].clone()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dw += torch.cat([dy2[lo:hi].t() @ R._tap_rows(xp, tap, c.T, Ho, Wo, c.stride)[order][lo:hi] for tap in taps], dim=1)
            db += dy2[lo:hi].sum(0)
        dwr, dbr = R.exact_weight_grad(name)
        assert dw.dtype == torch.float32 and torch.equal(dw.double(), d["dw_fill"].double() + dwr) and torch.equal(db.double(), d["db_fill"].double() + dbr)


# ------------------------------------------------------------------------------------------------ plans
def _fwd_args(c):
    return (c.N, c.T, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.stride, c.Cin + c.pads[0], c.Cout + c.pads[1])


def _dw_args(c):
    return (c.N, c.T, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.stride, c.Cin + c.pads[0], c.Cout + c.pads[3])


@pytest.mark.parametrize("name", list(R.CASES))
def test_written_plans_follow_the_tiling(name):
    """the hand-written plans restated with ceilings (forward) and their defining inequalities (dW), and the library's host-only queries
    under the forced modes agree with them"""
    from vt355 import ops
    c = R.CASES[name]
    M, Q = R.positions(c), c.k[0] * c.k[1] * c.k[2] * c.Cin
    up = lambda a, b: -(-a // b)
    assert c.Cin % 8 == 0 and all(p % 4 == 0 for p in c.pads) and c.pads[0] % 8 == 0 and (c.Cout + c.pads[3]) % 8 == 0
    if "f" in c.run or "x" in c.run:
        assert c.Cin % 64 == 0 and c.Cout % 4 == 0
        assert c.f128 == up(M, 128) * up(c.Cout, 128)
        assert (c.f320 is None) == (c.Cout % 320 != 0)
        if c.f320:
            tiles = up(M, 128) * (c.Cout // 320)
            grid = min(tiles, c.slots or 256)
            assert c.f320 == (grid, tiles, up(tiles, grid))
    if "x" in c.run:
        assert c.Cout % 64 == 0 and (c.stride == 1 or (c.H, c.W) == tuple(2 * v for v in R.case_hw(c)))
    assert c.d128[0] == up(c.Cout, 128) * up(Q, 128) and (c.d320 is None) == (c.Cout % 320 != 0)
    for plan, gran in ((c.d128, 64), (c.d320, 32)):
        if plan:
            tiles, splits, chunk = plan
            assert chunk % gran == 0 and (splits - 1) * chunk < M <= splits * chunk
    if c.d320:
        assert c.d320[0] == c.Cout // 320 * up(Q, 128)
    try:
        for kn, km in R.KERNELS.items():
            ops.conv_set_tile(km, c.slots if km == 2 else 0)
            if "f" in c.run:
                want = (2,) + c.f320 if km == 2 and c.f320 else (1, c.f128, c.f128, 1)
                assert ops.conv_plan(*_fwd_args(c)) == want
            if "x" in c.run:
                ops.conv_set_tile(km, 0)
                want = R.dx_plan(c, km) or R.dx_plan(c, 1)
                assert ops.conv_plan(c.N, c.T, c.H, c.W, c.Cout, c.Cin, c.k, c.pad, 1, c.Cout + c.pads[3], c.Cin + c.pads[1]) == want
            if "w" in c.run:
                want = (2,) + c.d320 + (1, 0) if km == 2 and c.d320 else (1,) + c.d128 + (0, 0)
                assert ops.conv_dw_plan(*_dw_args(c)) == want
    finally:
        ops.conv_set_tile(0)


def test_case_list_covers_what_it_claims():
    C = R.CASES
    fw = [C[n] for n in R.FWD_CASES]
    dw = [C[n] for n in R.DW_CASES]
    assert {R.positions(C[n]) for n in ("rows_128", "rows_129", "rows_255")} == {128, 129, 255}
    # tiles that straddle samples, T = 1, Wo = 1, H = W = 1, primes
    assert any(c.N >= 3 and R.positions(c) < 128 for c in fw) and any(c.T == 1 for c in fw) and any(R.case_hw(c)[1] == 1 for c in fw)
    assert any(c.H == 1 and c.W == 1 for c in fw)
    assert {7, 11, 13} <= {v for c in fw for v in (c.T,) + R.case_hw(c)} and any(R.case_hw(c)[0] * R.case_hw(c)[1] == 43 for c in fw)
    assert {4, 132, 320, 640} <= {c.Cout for c in fw} and {64, 128, 192, 320} <= {c.Cin for c in fw}
    assert {c.Cin for c in fw if c.f320} >= {64, 320}
    # every tap shape at stride 1 and at stride 2 with odd and with even H / W
    for k in (R.K33, R.K311, R.K111):
        assert any(c.k == k and c.stride == 1 for c in fw)
        assert {(c.H % 2, c.W % 2) for c in fw if c.k == k and c.stride == 2} >= {(1, 1), (0, 0)}
    # hand-over: slots 8 at 320 and 640 channels with both epilogues, workgroups walking three and two tiles; one odd grid on two column
    # tiles; the device's own grid with more tiles than workgroups
    ho = [c for c in fw if c.slots and c.f320[2] == 3 and c.f320[1] % c.f320[0]]
    assert {(c.Cout, c.res and c.sb) for c in ho if c.slots == 8} == {(320, False), (320, True), (640, False), (640, True)}
    assert any(c.slots % 2 == 1 and c.Cout == 640 for c in ho)
    assert any(c.slots == 0 and c.f320 and c.f320[1] > c.f320[0] == 256 for c in fw)
    assert any(c.pads[:3] != (0, 0, 0) and c.slots for c in fw)
    # dW: one split of <= 512 rows, several splits with a shorter ragged last one on either kernel, rows no multiple of 64 / 32
    assert any(c.d128[1] == 1 and R.positions(c) <= 512 for c in dw)
    assert any(c.d128[1] > 1 and R.positions(c) % c.d128[2] % 64 for c in dw)
    assert any(c.d320 and c.d320[1] == 1 and R.positions(c) < 256 and R.positions(c) % 32 for c in dw)
    assert any(c.d320 and c.d320[1] > 1 and R.positions(c) >= 2048 and R.positions(c) % c.d320[2] % 32 for c in dw)
    assert any(c.d320 and c.Cout == 640 for c in dw) and any(c.d320 and c.stride == 2 for c in dw)
    Q = lambda c: c.k[0] * c.k[1] * c.k[2] * c.Cin
    assert {192, 2880} <= {Q(c) for c in dw} and any(c.Cin % 128 and len(R.taps_of(c.k)) > 1 and Q(c) > 128 for c in dw)
    assert {(R.positions(c), c.Cout, c.Cin) for c in dw if c.run == "w"} >= {(1000, 320, 320), (77, 64, 1024), (300, 8, 72)}
    # input gradient: both strides on both kernels
    assert {(C[n].stride, kn) for n, kn in R.dx_pairs()} == {(1, "k128"), (2, "k128"), (1, "k320"), (2, "k320")}


def test_set_tile_slots_and_plans_on_the_host():
    """vt_conv_set_slots validates and changes nothing on an error; the queries launch nothing and report what the setting implies"""
    from vt355 import ops
    from vt355._lib import load_library
    geo = (2, 5, 10, 25, 64, 320)                        # handover_320: 2500 positions, 20 tiles of 128 x 320
    lib = load_library()
    try:
        ops.conv_set_tile(2, 8)
        assert ops.conv_plan(*geo) == (2, 8, 20, 3)
        for bad in (-1, 257, 1 << 20):
            assert lib.vt_conv_set_slots(bad) != 0
            assert ops.conv_plan(*geo) == (2, 8, 20, 3)
        with pytest.raises(RuntimeError):
            ops.conv_set_tile(3, 8)
        ops.conv_set_tile(2, 7)
        assert ops.conv_plan(*geo) == (2, 7, 20, 3)
        ops.conv_set_tile(2)                             # slots go back to the device's own
        assert ops.conv_plan(*geo) == (2, 20, 20, 1)
        ops.conv_set_tile(1, 8)                          # the cap does not reach the 128 x 128 kernel
        assert ops.conv_plan(*geo) == (1, 60, 60, 1) and ops.conv_dw_plan(*geo) == (1, 15, 5, 512, 0, 0)
        ops.conv_set_tile(0, 8)                          # nor the shape rule: 20 tiles are no full pass of the device
        assert ops.conv_plan(*geo)[0] == 1
        ops.conv_set_tile(0)
        assert ops.conv_plan(*geo) == (1, 60, 60, 1) and ops.conv_dw_plan(*geo) == (2, 5, 9, 288, 1, 0)
        for args in ((2, 5, 10, 25, 60, 320), (2, 5, 10, 25, 64, 322), (0, 5, 10, 25, 64, 320)):
            with pytest.raises(RuntimeError):
                ops.conv_plan(*args)
        with pytest.raises(RuntimeError):
            ops.conv_plan(*geo, kernel=(2, 3, 3))        # no temporal shrink
        with pytest.raises(RuntimeError):
            ops.conv_dw_plan(*geo, lddy=324)             # dy rows are 16-byte multiples
        # a Linear over more rows than one descriptor spans: 700 rows 5 MB apart run in chunks of 256
        assert ops.conv_dw_plan(1, 1, 1, 700, 384, 256, R.K111, R.P111, 1, 2_500_000, 2_500_000) == (1, 6, 1, 256, 0, 256)
    finally:
        ops.conv_set_tile(0)


def test_real_unet_convolution_list_and_rule_choices_on_256_cus():
    """REAL_CONVS holds every convolution build_structure gives the real VideoCrafter2 UNet, as often as it occurs, and (without a device
    the library assumes 256 CUs, an MI355X's) the kernels and splits written next to them"""
    from vt355 import ops
    counts = {}
    for conv in R.unet_convs(R.real_unet_structure(), 40, 64):
        counts[conv] = counts.get(conv, 0) + 1
    assert {k + (n,) for k, n in counts.items()} == set(R.REAL_CONVS)
    ops.conv_set_tile(0)
    assert R.real_unet_choices(ops) == R.REAL_CONVS
