"""Host side of the one-graph DDIM / PLMS loop (no GPU): the C entry is declared, exported and bound, and the two loop counters of
k22_debug_counter exist and start at zero."""
import os
import re
import subprocess
import sys

from kandinsky2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ddim_loop_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "k22.h")).read()
    assert re.search(r"\bint\s+k22_unet_ddim_loop\s*\(\s*K22UNet\s*\*\s*u\s*,\s*int\s+kind\b", hdr)
    m = re.search(r"enum\s*\{\s*K22_LOOP_DDIM\s*=\s*(\d+)\s*,\s*K22_LOOP_PLMS\s*=\s*(\d+)\s*\}", hdr)
    assert m and (int(m.group(1)), int(m.group(2))) == (_lib.K22_LOOP_DDIM, _lib.K22_LOOP_PLMS)
    assert hasattr(_lib.lib(), "k22_unet_ddim_loop")
    restype, argtypes = _lib.SIGNATURES["k22_unet_ddim_loop"]
    # one ctypes argument per declared parameter
    decl = re.search(r"int\s+k22_unet_ddim_loop\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(argtypes) == len(decl.split(","))
    # k22_unet_sample_loop keeps its signature
    assert len(_lib.SIGNATURES["k22_unet_sample_loop"][1]) == len(re.search(r"int\s+k22_unet_sample_loop\s*\(([^;]*)\)\s*;", hdr).group(1).split(",")) == 20


def test_a_null_handle_is_refused_without_a_device():
    L = _lib.lib()
    assert L.k22_unet_ddim_loop(None, _lib.K22_LOOP_DDIM, None, None, None, None, None, None, None, None, None, 5, 4.0, 1, None) == -1
    assert b"unet_ddim_loop" in L.k22_last_error()


def test_loop_counters_start_at_zero_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "from kandinsky2_amd import _lib\n"
            "L = _lib.lib()\n"
            "print(L.k22_debug_counter(b'loop_captures'), L.k22_debug_counter(b'loop_launches'), L.k22_debug_counter(b'nope'))\n")
    out = subprocess.run([sys.executable, "-c", code, ROOT], check=True, capture_output=True, text=True, cwd=ROOT).stdout
    assert out.split() == ["0", "0", "-1"], out


class _RecordingModel:
    """stands in for Text2ImUNetHIP: keeps what the samplers hand to ddim_loop"""

    def ddim_loop(self, kind, x, ts_rows, table, guidance_scale, noise_seq=None, **conditioning):
        self.got = dict(kind=kind, x=x, ts_rows=ts_rows, table=table, guidance=guidance_scale, noise_seq=noise_seq, conditioning=conditioning)
        return x + 1.0, x + 2.0


def test_samplers_hand_the_loop_its_calls_and_table_rows_in_execution_order():
    """Host side of whole_loop_graph=True for every loop length S = 5 can have (init_step 1 / 201 / 401 / None -> 1, 2, 3, 5 steps):
    timesteps of every model call newest first - PLMS repeats its second call's timestep, its own when it is the only step - and the
    schedule rows flipped to match; eta > 0 draws the noise of all steps by the stepwise path's randn_like calls."""
    import numpy as np
    import torch
    import kandinsky2_amd as k22
    old = k22.create_gaussian_diffusion(**k22.DIFFUSION_CONFIG_2_1)
    x_T = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(0))
    for init_step, steps in ((1, [1]), (201, [201, 1]), (401, [401, 201, 1]), (None, [801, 601, 401, 201, 1])):
        for cls, kind in ((k22.DDIMSamplerHIP, "ddim"), (k22.PLMSSamplerHIP, "plms")):
            m = _RecordingModel()
            s = cls(m, old, 4.0)
            out, aux = s.sample(5, 2, (4, 4, 4), conditioning={"full_emb": 1}, x_T=x_T, init_step=init_step, device="cpu", whole_loop_graph=True)
            calls = steps if kind == "ddim" else [steps[0], steps[min(1, len(steps) - 1)]] + steps[1:]
            g = m.got
            assert g["kind"] == kind and g["guidance"] == 4.0 and g["noise_seq"] is None and g["conditioning"] == {"full_emb": 1}
            assert g["ts_rows"].dtype == torch.float32 and g["ts_rows"].tolist() == [[float(c)] * 2 for c in calls]
            assert tuple(g["table"].shape) == (len(steps), 4) and g["table"].is_contiguous()
            assert np.array_equal(g["table"].numpy(), s.table[::-1])
            ac = old.alphas_cumprod
            assert np.array_equal(g["table"][:, 0].numpy(), ac[steps].astype(np.float32))       # a_t of the step executed k-th
            assert torch.equal(g["x"], x_T) and torch.equal(out, x_T + 1.0) and torch.equal(aux["pred_x0"][0], x_T + 2.0)
    m = _RecordingModel()
    torch.manual_seed(3)
    k22.DDIMSamplerHIP(m, old, 4.0).sample(5, 2, (4, 4, 4), x_T=x_T, eta=0.5, init_step=401, device="cpu", whole_loop_graph=True)
    torch.manual_seed(3)
    want = torch.stack([torch.randn_like(x_T) for _ in range(3)])
    assert torch.equal(m.got["noise_seq"], want) and m.got["table"][:, 2].abs().min().item() > 0     # sigma rows follow eta
