"""The CogVideoX sampler without a GPU: the fp64 restatement (tests/sampler_ref.py) against the in-tree twin's recorded numbers, the
scheduler's host side (timestep lists, coefficients, the first-order rule), the Philox-normal convention's statistics and key / stream
structure, the mutants the loop test's inputs have to separate, and the workflow's hooks."""
import json
import math
import os

import numpy as np
import pytest
import torch

import sampler_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "dpm_sampler.npz"))


def _same(got, ref, what):
    """finite reference: 1e-12 relative; an infinite or absent (nan) reference: the same infinity / absent"""
    if math.isnan(ref):
        assert got is None or math.isnan(got), f"{what}: {got} where the twin gives none"
    elif math.isinf(ref):
        assert got == ref, f"{what}: {got} against {ref}"
    else:
        assert abs(got - ref) <= 1e-12 * max(abs(ref), 1e-300), f"{what}: {got!r} against {ref!r}"


COLS = ("h", "r", "m1", "m2", "m3", "m4", "m_noise")


def test_restated_coefficients_match_the_twin(gold):
    abar, N = gold["abar"], 1000
    meta = json.loads(str(gold["meta"]))
    assert "self-oracle, reference-unpinned" in meta["timesteps"]
    for n in (50, 4):
        ts = [int(t) for t in gold[f"trailing{n}.timesteps"]]
        assert ts == R.timesteps(N, n, "trailing")
        for i, t in enumerate(ts):
            prev = t - N // n
            second = i > 0 and prev >= 0
            c = R.coefficients(abar[t], abar[prev] if prev >= 0 else 1.0, abar[ts[i - 1]] if second else None)
            for k, ref in zip(COLS, gold[f"trailing{n}.scalars"][i]):
                _same(c.get(k), float(ref), f"trailing{n} step {i} {k}")
    for (a_t, a_prev, a_back), row in zip(gold["edge.abar"], gold["edge.scalars"]):
        c = R.coefficients(a_t, a_prev, None if math.isnan(a_back) else a_back)
        for k, ref in zip(COLS, row):
            _same(c.get(k), float(ref), f"edge {a_t}->{a_prev} {k}")
    # the issue's table, to its printed digits
    e = gold["edge.scalars"]
    assert abs(e[0][3] + 0.547723) < 1e-6 and abs(e[0][6] - 0.836660) < 1e-6 and e[0][2] == 0
    assert abs(e[1][2] - 0.0824786) < 1e-7 and abs(e[1][3] + 0.903508) < 1e-6 and e[1][4] == 1 and e[1][5] == 0 and abs(e[1][6] - 0.308607) < 1e-6
    assert e[2][2] == 0 and e[2][3] == -1 and math.isinf(e[2][4]) and math.isinf(e[2][5]) and e[2][6] == 0


def test_restated_trajectory_matches_the_twin(gold):
    abar = gold["abar"]
    ts = [int(t) for t in gold["traj.timesteps"]]
    out = R.loop(gold["traj.x_init"], R.linear_denoiser(2, guided=False), abar, ts, 1000, 1.0, seed=0,
                 noise=list(gold["traj.noise"]) + [None])[:3]        # the fourth step (abar_prev = 1) is not part of the recording
    for i in range(3):
        err = np.abs(out[i] - gold["traj.x"][i].astype(np.float64)).max()
        print(f"transition {i}: max |restatement - twin (fp32)| = {err:.3g}")
        assert err <= 1e-6


def _schedulers():
    from vt355.scheduler import CogVideoXDPMScheduler
    for spacing in ("leading", "linspace", "trailing"):
        for zero_snr in (True, False):
            yield spacing, zero_snr, CogVideoXDPMScheduler(timestep_spacing=spacing, rescale_betas_zero_snr=zero_snr)


def test_host_coefficients_are_finite_and_match_the_restatement():
    for spacing, zero_snr, s in _schedulers():
        abar = s.alphas_cumprod.numpy()
        for n in range(1, 51):
            s.set_timesteps(n)
            ts = s.timesteps.tolist()
            assert ts == R.timesteps(1000, n, spacing)
            for i, t in enumerate(ts):
                c = s.step_coefficients(t, ts[i - 1] if i > 0 else None, have_old=i > 0)
                ref = R.step_plan(abar, ts, i, 1000, 1.0, i > 0)
                assert c["second_order"] == ref["second_order"]
                names = ("sa", "sb", "m1", "m2", "m_noise") + (("m3", "m4") if c["second_order"] else ())
                for k in names:
                    assert math.isfinite(c[k]), (spacing, zero_snr, n, i, k, c[k])
                    assert abs(c[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (spacing, zero_snr, n, i, k, c[k], ref[k])


def test_scheduler_surface_and_timestep_lists(tmp_path):
    from vt355.scheduler import CogVideoXDPMScheduler
    want = {("leading", 1): [0], ("leading", 4): [750, 500, 250, 0], ("linspace", 1): [0], ("linspace", 4): [999, 666, 333, 0],
            ("trailing", 1): [999], ("trailing", 4): [999, 749, 499, 249],
            ("leading", 50): list(range(980, -1, -20)), ("trailing", 50): list(range(999, 0, -20)),
            ("leading", 30): list(range(957, -1, -33)), ("linspace", 50): [int(round(999 * i / 49)) for i in range(49, -1, -1)]}
    for (spacing, n), ts in want.items():
        s = CogVideoXDPMScheduler(timestep_spacing=spacing)
        s.set_timesteps(n)
        assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == ts == R.timesteps(1000, n, spacing), (spacing, n)
        assert s.num_inference_steps == n
    for spacing in ("linspace", "trailing"):
        ts = R.timesteps(1000, 30, spacing)
        s = CogVideoXDPMScheduler(timestep_spacing=spacing); s.set_timesteps(30)
        assert s.timesteps.tolist() == ts and len(ts) == 30 and ts[0] == 999 and all(a > b for a, b in zip(ts, ts[1:]))
    assert R.timesteps(1000, 30, "trailing")[-1] == 32 and R.timesteps(1000, 30, "linspace")[-1] == 0
    s = CogVideoXDPMScheduler(timestep_spacing="leading", steps_offset=1); s.set_timesteps(4)
    assert s.timesteps.tolist() == [751, 501, 251, 1]
    s = CogVideoXDPMScheduler()
    assert s.config.timestep_spacing == "leading" and s.init_noise_sigma == 1.0 and s.order == 1 and s.num_inference_steps is None
    x = torch.ones(2)
    assert s.scale_model_input(x, 5) is x and float(s.final_alpha_cumprod) == 1.0
    assert float(CogVideoXDPMScheduler(set_alpha_to_one=False).final_alpha_cumprod) == float(s.alphas_cumprod[0])
    with pytest.raises(ValueError):
        s.step_coefficients(999)                                   # before set_timesteps
    with pytest.raises(ValueError):
        CogVideoXDPMScheduler(timestep_spacing="karras")
    (tmp_path / "scheduler_config.json").write_text(json.dumps({"_class_name": "CogVideoXDPMScheduler", "timestep_spacing": "trailing",
                                                                "steps_offset": 0, "set_alpha_to_one": True, "snr_shift_scale": 1.0}))
    s = CogVideoXDPMScheduler.from_pretrained(str(tmp_path))
    assert s.config.timestep_spacing == "trailing" and s.config.set_alpha_to_one is True and s.config.snr_shift_scale == 1.0


def test_last_step_is_first_order():
    from vt355.scheduler import CogVideoXDPMScheduler, dpm_coefficients
    s = CogVideoXDPMScheduler(timestep_spacing="trailing")
    for n in (4, 50):
        s.set_timesteps(n)
        ts = s.timesteps.tolist()
        c = s.step_coefficients(ts[-1], ts[-2], have_old=True)
        assert c["prev_timestep"] < 0 and c["second_order"] is False and c["m_noise"] == 0.0 and c["m2"] == -1.0 and c["m1"] == 0.0
        assert c["m3"] == 0.0 and c["m4"] == 0.0                  # nothing non-finite reaches the kernel
        raw = dpm_coefficients(float(s.alphas_cumprod[ts[-1]]), 1.0, float(s.alphas_cumprod[ts[-2]]))
        assert math.isinf(raw["m3"]) and math.isinf(raw["m4"])      # what second order would have handed it
        c1 = s.step_coefficients(ts[1], ts[0], have_old=True)      # behind the abar = 0 step: r = inf, still second order, finite
        assert c1["second_order"] is True and c1["m3"] == 1.0 and c1["m4"] == 0.0
        assert s.step_coefficients(ts[1], None, have_old=False)["second_order"] is False
        with pytest.raises(ValueError, match="timestep_back"):
            s.step_coefficients(ts[1], None, have_old=True)


def test_philox_normal_statistics_keys_and_streams():
    n = 1 << 20
    z = R.philox_normal(n, 1, seed=0x1234567, stream=0)[0]
    mean, var = z.mean(), z.var()
    print(f"2^20 draws: mean {mean:.3e} (sigma {1 / math.sqrt(n):.3e}), var - 1 {var - 1:.3e} (sigma {math.sqrt(2 / n):.3e}), max |z| {np.abs(z).max():.3f}")
    assert abs(mean) < 5 / math.sqrt(n) and abs(var - 1) < 5 * math.sqrt(2 / n)          # sd of the mean 1/sqrt(n), of the variance sqrt(2/n)
    assert np.isfinite(z).all() and np.abs(z).max() <= math.sqrt(2 * 24 * math.log(2)) + 1e-12      # u1 >= 2^-24
    a = R.philox_normal(37, 3, seed=99, stream=2)
    for b in range(3):
        assert np.array_equal(a[b], R.philox_normal(37, 1, seed=99 + b, stream=2)[0])
    assert np.array_equal(R.philox_normal(5, 1, seed=2 ** 64, stream=0), R.philox_normal(5, 1, seed=0, stream=0))    # keys wrap mod 2^64
    assert np.array_equal(a[:, :33], R.philox_normal(33, 3, seed=99, stream=2))          # a prefix does not depend on n
    s = [R.philox_normal(4096, 1, seed=7, stream=k)[0] for k in (0, 1, 2, 51)]
    for i in range(len(s)):
        for j in range(i + 1, len(s)):
            assert not np.intersect1d(s[i], s[j]).size                               # streams share no value, let alone a run of them
            assert abs(np.corrcoef(s[i], s[j])[0, 1]) < 5 / math.sqrt(4096)


def test_inputs_separate_every_mutant(gold):
    """each wrong loop of sampler_ref.MUTANTS moves the final latents of the tiny 4-step run by more than 10x the latent bar of the GPU loop
    test (one bf16 step + 1e-5), on the trailing list -- except the prev-from-list mutant, which IS the right loop there (1000 // 4 = 250 is
    the list's own spacing) and is separated on the linspace list, which the GPU loop test therefore runs too"""
    abar = gold["abar"]
    x = R.philox_normal(16 * 4 * 4 * 2, 2, seed=5, stream=0).reshape(2, 2, 16, 4, 4)
    den = R.linear_denoiser(2)
    ratios = {}
    for spacing in ("trailing", "linspace"):
        ts = R.timesteps(1000, 4, spacing)
        for dyn in (False, True):
            base = R.loop(x, den, abar, ts, 1000, 1.0, seed=11, g=6.0, dynamic=dyn)[-1]
            for m in R.MUTANTS:
                ratios[(spacing, dyn, m)] = R.separation(R.loop(x, den, abar, ts, 1000, 1.0, seed=11, g=6.0, dynamic=dyn, mutant=m)[-1], base)
    for k, r in ratios.items():
        print(f"{k[0]:9s} dynamic_cfg={k[1]!s:5s} {k[2]:18s} separation / bar = {r:.3g}")
    for (spacing, dyn, m), r in ratios.items():
        if spacing == "trailing" and m == "prev_from_list":
            assert r == 0.0
        else:
            assert r > 10, (spacing, dyn, m, r)


# ------------------------------------------------------------------ workflow hooks
def test_log_images_exists_only_with_a_decodable_vae(tmp_path, monkeypatch):
    import vae_decoder_ref as V
    from vt355.config import instantiate_from_config
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    node = V.make_workflow_dir(tmp_path / "a", with_decoder=True)
    monkeypatch.chdir(tmp_path / "a")
    wf = instantiate_from_config(node)
    assert hasattr(wf, "log_images") and callable(wf.log_images)
    assert not hasattr(wf, "vae_decoder")                           # resolving the attribute built nothing
    with pytest.raises(ValueError, match="timesteps"):
        wf.sample(prompt_embeds=torch.zeros(1, 4, 64), timesteps=[999, 500])
    with pytest.raises(ValueError, match="sample_precision"):
        wf.sample(prompt_embeds=torch.zeros(1, 4, 64), sample_precision="float16")
    node = V.make_workflow_dir(tmp_path / "b", with_decoder=False)
    monkeypatch.chdir(tmp_path / "b")
    wf = instantiate_from_config(node)
    assert not hasattr(wf, "log_images") and hasattr(wf, "sample")
    node["params"]["first_stage_config"] = None                    # no first_stage_config checkpoint at all
    assert not hasattr(instantiate_from_config(node), "log_images")


def test_i2v_sample_is_refused_by_name():
    from vt355.workflow import CogVideoXI2V
    wf = CogVideoXI2V.__new__(CogVideoXI2V)
    torch.nn.Module.__init__(wf)
    with pytest.raises(NotImplementedError, match="CogVideoXI2V.sample"):
        wf.sample(prompt_embeds=torch.zeros(1, 4, 64))
    assert not hasattr(wf, "log_images")
