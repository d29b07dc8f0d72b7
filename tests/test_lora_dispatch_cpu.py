"""Which rank-side kernels the CogVideoX engine calls, and with what: engine._lora_down / _lora_da / _lora_dx against the call
sequences recorded from the commit before the three helpers existed (tests/golden/lora_dispatch_calls.json: the four _lora_*
helpers and the two inline to_out.0 branches of that commit under the same recorders).  No GPU: the twelve ops.* wrappers are
replaced by recorders that keep the function name, every scalar argument (defaults filled in) and, of a tensor argument,
[storage_offset, shape, stride]."""
import inspect
import json
import os
from types import SimpleNamespace

import pytest
import torch

D, LAYERS, M, LAYER = 64, 2, 8, 1
DROP = (0.1, 1234567)
PRODUCTS = ("lora_down", "skinny_tn", "lora_up_add", "lora_down_wide", "lora_tn_wide", "lora_up_add_wide")
DA_OPS = ("skinny_tn", "skinny_tn_drop", "lora_tn_wide", "lora_tn_wide_drop")
# r = 4, 5: the three qkv adapters in one narrow call (3 r <= 16); 6, 16: one call each with zero_cols; 20, 80: wide, rp = 32 / 80 != r,
# lora_down_wide_drop takes the three adapters at once; 96, 128: it does not (rp > 80); (4, wide): VT355_LORA_WIDE=1, rp = 16
CASES = [(4, False), (5, False), (6, False), (16, False), (20, False), (80, False), (96, False), (128, False), (4, True)]

with open(os.path.join(os.path.dirname(__file__), "golden", "lora_dispatch_calls.json")) as _f:
    GOLDEN = json.load(_f)


def _desc(v):
    return [v.storage_offset(), list(v.shape), list(v.stride())] if isinstance(v, torch.Tensor) else v


@pytest.fixture
def calls(monkeypatch):
    from vt355 import ops
    log = []

    def recorder(name, sig):
        def rec(*a, **k):
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            log.append([name] + [_desc(v) for v in ba.arguments.values()])
        return rec
    for name in [p + s for p in PRODUCTS for s in ("", "_drop")]:
        monkeypatch.setattr(ops, name, recorder(name, inspect.signature(getattr(ops, name))))
    monkeypatch.setattr(ops, "lora_down_wide_drop_fits", lambda n, rp: n * (64 + rp) * 72 * 2 <= 65536 and n * rp <= 384)

    def take():
        out = json.loads(json.dumps(log))
        log.clear()
        return out
    return take


@pytest.mark.parametrize("need_dx", [True, False], ids=["dx", "no_dx"])
@pytest.mark.parametrize("drop", [None, DROP], ids=["nodrop", "drop"])
@pytest.mark.parametrize("r,forced_wide", CASES, ids=[f"r{r}{'_wide' if w else ''}" for r, w in CASES])
def test_rank_side_calls_match_the_recorded_sequences(calls, monkeypatch, r, forced_wide, drop, need_dx):
    from vt355 import engine
    from vt355.lora import LoraConfig, LoraState
    monkeypatch.setenv("VT355_LORA_WIDE", "1" if forced_wide else "0")
    model = SimpleNamespace(inner_dim=D, config=SimpleNamespace(num_layers=LAYERS), device="cpu")
    st = LoraState(model, LoraConfig(r=r, lora_alpha=float(r)))
    assert st.wide == (forced_wide or r > 16)
    want = GOLDEN[f"r{r}{'_wide' if forced_wide else ''}{'_drop' if drop else ''}"]
    bf = dict(dtype=torch.bfloat16)
    x1, dx1 = torch.empty(M, D + st.ext_qkv, **bf), torch.empty(M, D + st.ext_qkv, **bf)
    o, dO = torch.empty(M, D + st.ext_o, **bf), torch.empty(M, D + st.ext_o, **bf)

    engine._lora_down(st, LAYER, "qkv", x1, D, drop)
    assert calls() == want["down_qkv"]
    engine._lora_down(st, LAYER, "out", o, D, drop)
    assert calls() == want["down_out"]

    for proj, x, dxe, key in (("qkv", x1, dx1, "grads_qkv" if need_dx else "grads_qkv_no_dx"), ("out", o, dO, "grads_out")):
        engine._lora_da(st, LAYER, proj, x, dxe, D, drop)
        da = calls()
        if need_dx or proj == "out":            # to_out.0 always needs its dX
            engine._lora_dx(st, LAYER, proj, dxe, D, drop)
        dx = calls()
        assert da == [c for c in want[key] if c[0] in DA_OPS]
        assert dx == [c for c in want[key] if c[0] not in DA_OPS]
        # The recorded commit interleaved the per-adapter dA and dX calls of the narrow ranks 6..16 (dA_q, dX_q, dA_k, ...); the helpers
        # issue a product's calls together.  The calls are independent (dA reads x and the extension columns of dxe, dX writes only
        # the base columns of dxe), and everywhere else the whole sequence is the recorded one.
        if not (proj == "qkv" and need_dx and not st.wide and 3 * r > 16):
            assert da + dx == want[key]
