"""Inputs, the host model and the wrong variants of k22_sampler_step_groups (csrc/sampler.hip: one sampler_threshold_kernel workgroup per
threshold group, sampler_final_kernel reading the s of every row's group), for tests/test_sampler_groups_cpu.py and
tests/test_sampler_groups_gpu.py.  The select itself, its references, bounds and cases are tests/sampler_ref.py's; this module only lays
several of its images out in one batch.

  half = use_cfg ? N / 2 : N          group j = rows j g .. (j + 1) g - 1 of the cond half and their uncond partners
  s_j = max(percentile_99.5(|x0[row j g]|), 1)          row n is clamped and divided by s_{(n % half) / g}

An item uses sampler_ref.SELECT_ROW and model_out = 0 with a clamp that clamps nothing: x0_buf = x exactly, so every key is what the item wrote
and sampler_ref.dispatch labels the path every group's workgroup takes.  The source row of group j is one of sampler_ref's select cases - clamped
on the host where the case asks for it - times a scale of its own (GROUP_PLAN); every other row is other Gaussian values.
"""
import functools

import numpy as np
import torch

import sampler_ref as sp
from kandinsky2_amd.diffusion import percentile_index

# (N, HW, g, use_cfg) and why each is there
ITEMS = ((8, 2304, 1, 1),     # 4 groups, KPT 16, the filtered path
         (8, 255, 2, 1),      # 2 groups, KPT 4, n not a multiple of 1024
         (6, 1025, 1, 1),     # 3 groups, an odd count
         (4, 9216, 1, 1),     # the production KPT 36
         (4, 16385, 1, 1),    # the generic re-read path: the row offset applies to its memory reads too
         (2, 1, 1, 1),        # n = 4, k_hi at the end
         (3, 255, 1, 0),      # no CFG
         (8, 2304, 4, 1))     # one group
# group j -> (case of sampler_ref, scale): group 0 above 1, group 1 below 1 (s clamped to 1), group 2 the sample that misleads the pivot (the
# fall-back where the filter runs), group 3 a tie across the ranks lo - 3 .. lo + 3
GROUP_PLAN = (("gauss_open", 2.5), ("gauss_open", 0.4), ("sample_large", 1.0), ("tie_straddle", 1.3))
SMALL_CASE = "ulp_ramp_mid"          # the case of every group where the image is too small for the statistical ones (sampler_ref.case_applies)
MUTANTS = ("row_0", "source_plus_1", "no_mod")


def layout(N, g, use_cfg):
    """-> (half, number of groups)"""
    half = N // 2 if use_cfg else N
    assert half % g == 0
    return half, half // g


def group_case(j, n):
    case, scale = GROUP_PLAN[j]
    if not sp.case_applies(case, n):
        case = "tie_above" if sp.case_applies("tie_above", n) else SMALL_CASE
    return case, scale


@functools.lru_cache(maxsize=None)
def item_input(N, HW, g, use_cfg):
    """the operands of one item: x [N][4][HW], model_out = 0, noise; clamp = sampler_ref.WIDE"""
    n = 4 * HW
    half, G = layout(N, g, use_cfg)
    rng = np.random.default_rng(104729 * N + 31 * HW + g)
    rows = [(0.8 * rng.standard_normal(n)).astype(np.float32) for _ in range(N)]
    for j in range(G):
        case, scale = group_case(j, n)
        img, clamp = sp._image0(case, n, np.random.default_rng(7919 * sp.CASES.index(case) + HW + 1000 * j))
        rows[j * g] = (np.clip(img, -clamp, clamp) * np.float32(scale)).astype(np.float32)
    return {"x": torch.from_numpy(np.stack(rows).reshape(N, 4, HW)), "mo": torch.zeros(N, 8, HW),
            "noise": torch.from_numpy(rng.standard_normal((N, 4, HW)).astype(np.float32)), "clamp": sp.WIDE}


def group_s(x0, N, g, use_cfg, emul=False):
    """[G] float32: the reference s of every group from the stored x0 [N][4 HW] - numpy's percentile of row j g evaluated as sampler_ref.s_ref does,
    or (emul) sampler_ref.select_emul, the host model of the kernel, on that row"""
    half, G = layout(N, g, use_cfg)
    lo, gamma = percentile_index(x0.shape[1])
    return np.array([sp.select_emul(x0[j * g:j * g + 1], lo, gamma) if emul else sp.s_ref(x0[j * g]) for j in range(G)], dtype=np.float32)


def row_s(S, N, g, use_cfg):
    """[N] float32: the s every row is clamped and divided by"""
    half, G = layout(N, g, use_cfg)
    return np.array([S[(r % half) // g] for r in range(N)], dtype=np.float32)


def mutant_row_s(x0, N, g, use_cfg, mutant):
    """[N] float32: what one deliberately wrong implementation applies to every row (NaN: it reads a float of s_buf that no workgroup wrote)
      row_0          every group's threshold from row 0: the kernels before the groups
      source_plus_1  group j selects over row j g + 1
      no_mod         the final kernel indexes s_buf by n / g without the % half"""
    half, G = layout(N, g, use_cfg)
    S = group_s(x0, N, g, use_cfg)
    if mutant == "row_0":
        return np.full(N, S[0], dtype=np.float32)
    if mutant == "source_plus_1":
        return row_s(np.array([sp.s_ref(x0[min(j * g + 1, N - 1)]) for j in range(G)], dtype=np.float32), N, g, use_cfg)
    assert mutant == "no_mod"
    return np.array([S[r // g] if r // g < G else np.nan for r in range(N)], dtype=np.float32)


def final_ref(x0_buf, S, d, row, N, g, use_cfg, dtype=torch.float64):
    """sampler_ref.final_ref with each row's own s -> (x_out, x0_out, S of x_out), [N][4][HW]"""
    per_row = row_s(S, N, g, use_cfg)
    outs = [sp.final_ref(x0_buf[r:r + 1], per_row[r], {k: (v[r:r + 1] if torch.is_tensor(v) else v) for k, v in d.items()}, row, dtype=dtype)
            for r in range(N)]
    return tuple(torch.cat([o[k] for o in outs], 0) for k in range(3))
