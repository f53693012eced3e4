#!/usr/bin/env python
"""Goldens of the prior's DDIM route, made by running the REFERENCE's own PriorDiffusionModel.forward with
timestep_respacing="ddimN" (kandinsky2/model/prior.py:318-384 -> GaussianDiffusion.ddim_sample_loop) on seeded weights and inputs.
Build-container only: it needs the reference tree (oracle.ref_loader).

    python tools/make_golden_prior_ddim.py          # tables + prior_tiny_ddim.pt (seconds)
    python tools/make_golden_prior_ddim.py --full   # also prior_full_ddim.pt (the 1.02 B-parameter prior on the CPU: a minute)

Writes data only, under tests/golden/:
    ref_prior_ddim_tables.json   per respacing string: num_timesteps, timestep_map and the reference diffusion's float64 alphas_cumprod,
                                 alphas_cumprod_prev, sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod as float.hex() strings
    prior_tiny_ddim.pt           tiny_prior_hparams(), bs = 2: final samples of four (string, eta) cases + one mid-loop ddim_sample record
    prior_full_ddim.pt           PRIOR_HPARAMS_2_1, bs = 2: the final sample of ("ddim5", eta 0)
The weights (init_prior_state_dict(hp, seed=0)) and the conditioning (oracle.make_golden.prior_inputs) are re-drawn from their seeds by
the tests; x_T and the per-step noise of a case come from its `noise_seed`:  g = Generator().manual_seed(noise_seed);
x_T = randn(N, 768, generator=g); noise_seq = randn(num_timesteps, N, 768, generator=g).
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kandinsky2_amd as k22  # noqa: E402
from oracle import ref_loader  # noqa: E402
from oracle.make_golden import prior_inputs  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
TABLE_STRINGS = ("ddim3", "ddim10", "ddim25", "ddim30", "ddim1000")
TINY_CASES = (("ddim5", 0.0, 101), ("ddim30", 0.0, 102), ("ddim5", 1.0, 103), ("ddim3", 0.5, 104))   # (string, eta, noise_seed)
RECORD_CASE, RECORD_STEP = ("ddim5", 1.0), 2   # the third step run of ddim5 (schedule index 2): sigma, direction and noise all live


def tables():
    mc = ref_loader.ref("model.model_creation")
    out = {}
    for r in TABLE_STRINGS:
        d = mc.create_gaussian_diffusion(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing=r))
        out[r] = dict(num_timesteps=int(d.num_timesteps), timestep_map=[int(t) for t in d.timestep_map],
                      **{n: [float(v).hex() for v in getattr(d, n)] for n in
                         ("alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")})
        print(f"{r}: {d.num_timesteps} steps, timestep_map {out[r]['timestep_map'][:3]} ... {out[r]['timestep_map'][-1]}")
    with open(os.path.join(GOLD, "ref_prior_ddim_tables.json"), "w") as f:
        json.dump(out, f)


def reference_prior(hp, bs):
    pr = ref_loader.ref("model.prior")
    conf = types.SimpleNamespace(model=types.SimpleNamespace(hparams=types.SimpleNamespace(**hp)),
                                 diffusion=types.SimpleNamespace(**k22.PRIOR_DIFFUSION_2_1))

    class Tok:  # only used for the (unused here) cf_token buffers
        def padded_tokens_and_mask(self, texts, ctx):
            return torch.zeros(1, ctx, dtype=torch.long), torch.ones(1, ctx, dtype=torch.bool)

    cm, cs, txt_feat, txt_seq, mask, _x, _g = prior_inputs(bs)
    m = pr.PriorDiffusionModel(conf, Tok(), cm, cs).eval()
    m.model.load_state_dict(k22.init_prior_state_dict(hp, seed=0), strict=True)
    return m, (txt_feat, txt_seq, mask)


def run_case(m, cond, scales, respacing, eta, noise_seed, record_step=None):
    """The reference's forward with eta handed to its own ddim_sample_loop and its randn / randn_like replaced by the seeded draws.
    record_step: the execution-order number of the ddim_sample call to record (x, guided model_out, noise, sample, pred_xstart, index)."""
    gd = ref_loader.ref("model.gaussian_diffusion")
    mc = ref_loader.ref("model.model_creation")
    T = mc.create_gaussian_diffusion(**dict(k22.PRIOR_DIFFUSION_2_1, timestep_respacing=respacing)).num_timesteps
    N = cond[0].shape[0]
    g = torch.Generator().manual_seed(noise_seed)
    x_T, noise_seq = torch.randn(N, 768, generator=g), torch.randn(T, N, 768, generator=g)
    record, calls = {}, [0]
    get_sample_fn = m.get_sample_fn

    def with_eta(r):
        loop = get_sample_fn(r)   # diffusion.ddim_sample_loop, bound
        diffusion, step = loop.__self__, loop.__self__.ddim_sample

        def recording_step(model, x, t, **kw):
            k, seen = calls[0], {}
            calls[0] += 1

            def model_seen(x_, ts_, **mk):
                seen["out"] = model(x_, ts_, **mk)
                return seen["out"]

            out = step(model_seen, x, t, **kw)
            if k == record_step:
                record.update(index=int(t[0]), x=x.clone(), model_out=seen["out"].clone(), noise=noise_seq[k].clone(),
                              sample=out["sample"].clone(), pred_xstart=out["pred_xstart"].clone())
            return out

        diffusion.ddim_sample = recording_step
        return lambda *a, **kw: loop(*a, eta=eta, **kw)

    it = iter(noise_seq)
    o1, o2 = gd.th.randn_like, gd.th.randn
    gd.th.randn_like = lambda t_: next(it).to(t_)
    gd.th.randn = lambda *shape, **kw: x_T.clone()
    m.get_sample_fn = with_eta
    try:
        with torch.no_grad():
            sample = m(*cond, scales, timestep_respacing=respacing)
    finally:
        gd.th.randn_like, gd.th.randn = o1, o2
        del m.get_sample_fn
    assert calls[0] == T and next(it, None) is None, "one randn_like per step, as many steps as the schedule has"
    print(f"  {respacing} eta {eta}: {T} steps, sample absmax {sample.abs().max():.3f}")
    return dict(respacing=respacing, eta=eta, noise_seed=noise_seed, num_timesteps=T, sample=sample.clone()), record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    tables()
    bs = 2
    scales = torch.tensor(([4.0, 2.5, 1.0, 7.0] * bs)[:bs])
    hp = k22.tiny_prior_hparams()
    m, cond = reference_prior(hp, bs)
    cases, record = [], None
    print("prior_tiny_ddim:")
    for r, eta, seed in TINY_CASES:
        c, rec = run_case(m, cond, scales, r, eta, seed, RECORD_STEP if (r, eta) == RECORD_CASE else None)
        cases.append(c)
        if rec:
            record = dict(rec, respacing=r, eta=eta, scales=scales.clone())
    assert record is not None and record["index"] == 2
    torch.save(dict(name="prior_tiny_ddim", hp=hp, bs=bs, seed_w=0, scales=scales, cases=cases, record=record),
               os.path.join(GOLD, "prior_tiny_ddim.pt"))
    if a.full:
        hp = dict(k22.PRIOR_HPARAMS_2_1)
        m, cond = reference_prior(hp, bs)
        print("prior_full_ddim:")
        c, _ = run_case(m, cond, scales, "ddim5", 0.0, 105)
        torch.save(dict(name="prior_full_ddim", hp=hp, bs=bs, seed_w=0, scales=scales, cases=[c]), os.path.join(GOLD, "prior_full_ddim.pt"))


if __name__ == "__main__":
    main()
