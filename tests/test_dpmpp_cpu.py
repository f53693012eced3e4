"""Host side of the DPM-Solver++ sampler (no GPU): the production coefficient table (kandinsky2_amd.sampling.dpmpp_table) on a model
whose probability-flow ODE is solved in closed form, the teeth of that check, the order-1 rows against DDIM's coefficients, the two
grids, and the per-element bound of the step kernel (tests/dpmpp_ref.py) around torch's own fp32 evaluation.  Every figure in a
docstring was measured with the code of this file; every assertion is a condition stated before it was."""
import numpy as np
import pytest
import torch

import dpmpp_ref as R
import kandinsky2_amd as k22
from kandinsky2_amd import _lib, sampling

AC = R.schedule_2_1()


def _err(grid, order=2, mut=None, lof=True):
    """toy-model error of the PRODUCTION table (mut None) or of a mutant of the restatement on (ac_s, ac_t)"""
    a, b = grid
    table, orders = sampling.dpmpp_table(a, b, order, lof) if mut is None else R.table_ref(a, b, order, lof, mut)
    return R.toy_error(table, orders, a, b)


def _toy_conditions(mut=None):
    """the three conditions of the toy model -> list of (name, holds, figures)"""
    e2 = [_err(R.real_grid(AC, n), 2, mut) for n in (20, 40, 80)]
    e1 = [_err(R.real_grid(AC, n), 1, mut) for n in (20, 40, 80)]
    few = _err(R.integer_grid(AC, sampling.dpmpp_grid(AC, 20, "logsnr")), 2, mut)
    many = _err(R.integer_grid(AC, sampling.dpmpp_grid(AC, 100, "uniform")), 1)          # the yardstick: production order 1 = DDIM
    return [("order 2 ratios >= 3", e2[0] / e2[1] >= 3 and e2[1] / e2[2] >= 3, e2),
            ("order 1 ratios in [1.7, 2.3]", all(1.7 <= r <= 2.3 for r in (e1[0] / e1[1], e1[1] / e1[2])), e1),
            ("2M logsnr 20 beats order 1 uniform 100", few < many, (few, many))]


# ---- 1. the toy model ------------------------------------------------------------------------------------------------------------------
def test_production_table_converges_at_its_order_on_the_closed_form_model():
    """Measured: order 2 errors 4.19e-3 / 1.14e-3 / 2.91e-4 at 20 / 40 / 80 steps uniform in log-SNR (ratios 3.7, 3.9); order 1
    5.59e-2 / 2.86e-2 / 1.44e-2 (1.96, 1.98); 2M on "logsnr" S = 20: 4.08e-3 against 1.92e-2 of order 1 on "uniform" S = 100 (4.7x)."""
    for name, holds, figures in _toy_conditions():
        print(name, figures)
        assert holds, (name, figures)


def test_production_table_equals_the_restatement():
    for power, n, order, lof in ((1.0, 20, 2, True), (1.5, 7, 2, False), (1.5, 3, 1, True)):
        a, b = R.real_grid(AC, n, power)
        t, o = sampling.dpmpp_table(a, b, order, lof)
        tr, orr = R.table_ref(a, b, order, lof)
        assert t.dtype == np.float64 and t.shape == (n, 5) and list(o) == list(orr)
        assert np.all(np.abs(t - tr) <= 1e-12 * np.abs(tr)), np.abs(t - tr).max()


# ---- 2. teeth --------------------------------------------------------------------------------------------------------------------------
def test_wrong_r_and_wrong_history_sign_show_on_the_non_uniform_grid():
    """u^1.5 grid, 40 steps.  Measured: correct 4.51e-4, r inverted 2.10e-3 (4.65x), history sign flipped 6.00e-2 (133x)."""
    g = R.real_grid(AC, 40, 1.5)
    ok, r_inv, sign = _err(g), _err(g, mut="r_inverted"), _err(g, mut="history_sign")
    print(f"correct {ok:.3e}, r inverted {r_inv:.3e} ({r_inv / ok:.2f}x), history sign {sign:.3e} ({sign / ok:.1f}x)")
    assert ok <= r_inv / 3 and ok <= sign / 50


@pytest.mark.parametrize("mut", R.TABLE_MUTANTS)
def test_each_mutant_of_the_restatement_fails_the_toy_model(mut):
    """h_sign, cx_inverted and exp_for_expm1 do not converge at all (errors ~1 and ~500); history_on_step0 (step 0 reads an empty history
    slot) costs the second order its constant: ratios 3.16 and 2.99 against the 3 required."""
    res = _toy_conditions(mut)
    print(mut, [(n, h, f) for n, h, f in res])
    assert not all(h for _, h, _ in res)


# ---- 3. order-1 rows are DDIM ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 50, 100])
def test_order_1_rows_equal_ddim_coefficients(S):
    """The eta = 0 DDIM update x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) e with e = (x - sqrt(a_t) x0) / sqrt(1 - a_t), in x and x0:
    c_x = sqrt((1 - a_prev) / (1 - a_t)), c_0 = sqrt(a_prev) - c_x sqrt(a_t); a_t / a_prev are make_schedule's, in float64."""
    old = k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)
    sm = k22.DDIMSamplerHIP(None, old, 4.0)
    sm.make_schedule(S)
    steps, ac = sm.ddim_timesteps, old.alphas_cumprod
    assert np.array_equal(ac, AC)
    a_t = ac[steps][::-1]
    a_prev = np.asarray([ac[0]] + ac[steps[:-1]].tolist())[::-1]
    assert np.array_equal(a_t.astype(np.float32), sm.table[::-1, 0]) and np.array_equal(a_prev.astype(np.float32), sm.table[::-1, 1])
    table, orders = sampling.dpmpp_table(a_t, a_prev, solver_order=1)
    c_x = np.sqrt((1 - a_prev) / (1 - a_t))
    want = np.stack([np.sqrt(a_t), np.sqrt(1 - a_t), c_x, np.sqrt(a_prev) - c_x * np.sqrt(a_t), np.zeros_like(a_t)], 1)
    rel = np.abs(table - want) / np.maximum(np.abs(want), 1e-300)
    print(f"S={S}: worst relative difference {rel.max():.2e}")
    assert list(orders) == [1] * len(a_t) and np.all(table[:, 4] == 0.0)
    assert rel.max() <= 1e-12


# ---- 4. grids and orders ---------------------------------------------------------------------------------------------------------------
def test_grids():
    old = k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)
    sm = k22.DDIMSamplerHIP(None, old, 4.0)
    for S, init in ((5, None), (50, None), (100, 400), (7, 1)):
        sm.make_schedule(S, init_step=init)
        assert np.array_equal(sampling.dpmpp_grid(AC, S, "uniform", init), sm.ddim_timesteps[::-1])
    for S, n in ((1, 1), (6, 6), (20, 20)):
        ts = sampling.dpmpp_grid(AC, S, "logsnr")
        assert ts.dtype.kind == "i" and len(ts) == n and ts[0] == 999 and ts.min() >= 1 and np.all(np.diff(ts) < 0), ts
    assert len(sampling.dpmpp_grid(AC, 50, "logsnr")) == 48            # near t = 999 the schedule is coarser in lambda than the targets
    full, cut = sampling.dpmpp_grid(AC, 20, "logsnr"), sampling.dpmpp_grid(AC, 20, "logsnr", init_step=400)
    assert list(cut) == [t for t in full if t <= 400] and 0 < len(cut) < len(full)
    with pytest.raises(ValueError):
        sampling.dpmpp_grid(AC, 20, "quadratic")


def test_orders():
    for n in (1, 2, 3, 6):
        a, b = R.real_grid(AC, n)
        want = {1: [1], 2: [1, 1], 3: [1, 2, 1], 6: [1, 2, 2, 2, 2, 1]}[n]
        t, o = sampling.dpmpp_table(a, b)
        assert list(o) == want and all((t[k, 4] == 0.0) == (want[k] == 1) for k in range(n))
        t, o = sampling.dpmpp_table(a, b, lower_order_final=False)
        assert list(o) == [1] + [2] * (n - 1) and all(t[k, 4] != 0.0 for k in range(1, n))
        t, o = sampling.dpmpp_table(a, b, solver_order=1)
        assert list(o) == [1] * n and np.all(t[:, 4] == 0.0)
    with pytest.raises(ValueError):
        sampling.dpmpp_table(*R.real_grid(AC, 3), solver_order=3)


def test_sampler_class_refuses_before_it_touches_the_gpu():
    old = k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)
    sm = k22.DPMSolverSamplerHIP(None, old, 4.0)
    for kw in (dict(eta=0.5), dict(solver_order=3), dict(solver_order=0), dict(discretize="quadratic")):
        with pytest.raises(ValueError):
            sm.sample(6, 2, (4, 16, 16), device="cpu", **kw)
    sm.make_dpm_schedule(50)
    assert len(sm.timesteps) == 48 and sm.dpm_table.shape == (48, 5) and list(sm.orders) == [1] + [2] * 46 + [1]
    assert issubclass(k22.DPMSolverSamplerHIP, k22.DDIMSamplerHIP)


# ---- 5. the step bound -----------------------------------------------------------------------------------------------------------------
def _rows():
    """(row, order) of the first (t = 999: alpha_s = 0.040, the largest 1 / alpha_s there is), a middle and the last step of the real S = 20
    table"""
    ts = sampling.dpmpp_grid(AC, 20, "logsnr")
    table, orders = sampling.dpmpp_table(*R.integer_grid(AC, ts), lower_order_final=False)
    assert 0.03 < table[0, 0] < 0.08 and table[19, 0] > 0.99
    return [(table[0], 1), (table[10], 2), (table[19], 2)]


@pytest.mark.parametrize("use_cfg", [0, 1])
def test_fp32_evaluation_lies_inside_the_derived_bound_and_the_mutants_outside(use_cfg):
    d = R.step_inputs(4, 257, seed=1)
    for row, order in _rows():
        prev = d["x0_prev"] if order == 2 else None
        ref, x0, S, S0 = R.step64(d["x"], d["model_out"], prev, row, 4.0, use_cfg)
        out32, x032, _, _ = R.step64(d["x"], d["model_out"], prev, row, 4.0, use_cfg, dtype=torch.float32)
        assert out32.dtype == torch.float32
        print(f"cfg {use_cfg} alpha_s {row[0]:.3f} order {order}: fp32 / bound  out {R.worst_ratio(out32, ref, R.bound_out(S)):.3f}  "
              f"x0 {R.worst_ratio(x032, x0, R.bound_x0(S0)):.3f}")
        assert R.violations(out32, ref, R.bound_out(S)) == 0 and R.violations(x032, x0, R.bound_x0(S0)) == 0
        for mut in R.STEP_MUTANTS:
            if (mut == "guidance_wrong_half" and not use_cfg) or (mut in ("x0_prev_other_sample", "c0_c1_swapped") and order == 1):
                continue                                   # the mutant does not touch this case
            bad, bad0, _, _ = R.step64(d["x"], d["model_out"], prev, row, 4.0, use_cfg, mut=mut)
            n_bad = R.violations(bad, ref, R.bound_out(S)) + R.violations(bad0, x0, R.bound_x0(S0))
            assert n_bad > 0.5 * ref.numel(), (mut, n_bad)


# ---- 6. the C entries check their arguments before they touch a device -------------------------------------------------------------------
def test_c_entries_refuse_null_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.k22_dpmpp_step(None, None, None, None, 4.0, 1, None, None, 2, 16, None) == -1 and b"dpmpp_step" in L.k22_last_error()
    assert L.k22_unet_dpmpp_loop(None, None, None, None, None, None, None, None, None, 1, 4.0, 1, None) == -1
    assert b"unet_dpmpp_loop" in L.k22_last_error()
