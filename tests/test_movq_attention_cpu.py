"""The fused MoVQ attention on the host: the float64 bound of movq_attn_ref against a float32 emulation of the kernel's scheme and against
its mutants, torch's own fp32 error (the yardstick behind the bound's c), and the attention= / movq_attention= plumbing of the Python layer
on recording fakes (device "cpu": no GPU, and no native code is run)."""
import pytest
import torch

import movq_attn_ref as mq
from kandinsky2_amd import _lib, movq, pipeline, pipeline22
from kandinsky2_amd.native import NativeEngine, layout_arena


# ---- (a) the scheme stays inside the bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mq.DTYPES, ids=lambda d: mq.DT_NAME[d])
def test_emulated_scheme_is_inside_the_bound(dtype):
    worst = 0.0
    for c, fam in mq.pairs():
        ref, bnd, (q, k, v, bias, _A, _amp) = mq.ref_and_bound(c, fam, dtype)
        out = mq.emulate(q, k, v, bias, dtype).double()
        r = mq.worst_ratio(out, ref, bnd)
        worst = max(worst, r)
        assert r <= 1.0, (mq.case_id(c), fam, r)
    print(f"emulation {mq.DT_NAME[dtype]}: worst |out - ref| / bound = {worst:.3f}")


# ---- (b) every mutant leaves the bound -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", mq.MUTANTS)
def test_every_mutant_leaves_the_bound_for_every_type(mut):
    for dtype in mq.DTYPES:
        caught = []
        for c, fam in mq.pairs():
            ref, bnd, _ = mq.ref_and_bound(c, fam, dtype)
            wrong = mq.mutant_ref(c, fam, dtype, mut)
            # as a kernel with this mistake would store it: the mutant's float64 value rounded to the type
            r = mq.worst_ratio(wrong.to(mq.hp.tdt(dtype)).double(), ref, bnd)
            if r > 1.0:
                caught.append((mq.case_id(c), fam, round(r, 1)))
        print(f"{mut} {mq.DT_NAME[dtype]}: rejected by {len(caught)} of {len(mq.pairs())} case x family pairs")
        assert caught, (mut, mq.DT_NAME[dtype])


# ---- (c) the yardstick -----------------------------------------------------------------------------------------------------------------
def test_yardstick_torch_fp32_stays_under_c():
    per_family = {}
    for dtype in mq.DTYPES:
        for c, fam in mq.pairs():
            ref, _bnd, (q, k, v, bias, A, amp) = mq.ref_and_bound(c, fam, dtype)
            y = mq.yardstick(mq.plain32(q, k, v, bias), ref, A, amp)
            per_family[fam] = max(per_family.get(fam, 0.0), y)
            assert y < mq.MQ_C, (mq.case_id(c), fam, y)
    print("yardstick (CPU) " + "   ".join(f"{f} {per_family[f]:.2f}" for f in mq.FAMILIES))


# ---- (d) host logic on recording fakes -------------------------------------------------------------------------------------------------
class FakeMoVQEntries:
    """create / destroy / plan / bind / set_attention of the MoVQ family, recording"""

    def __init__(self):
        self.calls = []

    def create(self, cfg, weights, n, handle):
        handle._obj.value = 0x2000
        return 0

    def destroy(self, handle):
        self.calls.append(("destroy",))

    def plan(self, handle, B, h, w, size):
        self.calls.append(("plan", B, h, w))
        size._obj.value = 512
        return 0

    def bind(self, handle, ptr, nbytes):
        self.calls.append(("bind",))
        return 0

    def set_attention(self, handle, mode):
        self.calls.append(("set_attention", mode))
        return 0

    def entries(self):
        return self.create, self.destroy, self.plan, self.bind, self.set_attention


def _with_fake_engine(module, kind):
    fake = FakeMoVQEntries()
    arena, table = layout_arena({"w": torch.ones(4)}, "cpu")
    module._engines["movq"] = NativeEngine(movq.movq_family(kind, fake.entries()), _lib.K22MoVQConfig(), arena, table)
    return fake


@pytest.mark.parametrize("cls,kind", [(movq.MoVQDecoderHIP, "movq"), (movq.MoVQEncoderHIP, "movq_encoder")])
def test_attention_keyword_reaches_the_handle_before_the_plan_and_keys_it(cls, kind):
    assert cls().attention == "auto"                                                  # the default
    m = cls(attention="fused")
    fake = _with_fake_engine(m, kind)
    m._ensure_plan(1, 8, 8)
    assert fake.calls == [("set_attention", 2), ("plan", 1, 8, 8), ("bind",)]
    m._ensure_plan(1, 8, 8)                                                           # same key: nothing more
    assert len(fake.calls) == 3
    m.attention = "scores"                                                            # assigned afterwards: the next call plans again
    m._ensure_plan(1, 8, 8)
    assert fake.calls[3:] == [("set_attention", 1), ("plan", 1, 8, 8), ("bind",)]
    m.attention = "auto"
    m._ensure_plan(2, 8, 8)
    assert fake.calls[6:] == [("set_attention", 0), ("plan", 2, 8, 8), ("bind",)]
    assert m._engines["movq"].plan_key == (2, 8, 8, 0)


@pytest.mark.parametrize("cls", [movq.MoVQDecoderHIP, movq.MoVQEncoderHIP])
def test_attention_rejects_anything_but_the_three_modes(cls):
    for bad in ("flash", "", None, 2):
        with pytest.raises(ValueError):
            cls(attention=bad)
    m = cls()
    with pytest.raises(ValueError):
        m.attention = "Fused"
    assert m.attention == "auto"                                                      # a refused assignment changes nothing


def test_a_refused_mode_fails_the_plan_before_it_is_built(monkeypatch):
    monkeypatch.setattr(_lib, "check", lambda rc: (_ for _ in ()).throw(RuntimeError(f"k22 error {rc}")) if rc else None)   # no library on the host
    m = movq.MoVQDecoderHIP()
    fake = FakeMoVQEntries()
    fake.set_attention = lambda handle, mode: -1
    m._engines["movq"] = NativeEngine(movq.movq_family("movq", fake.entries()), _lib.K22MoVQConfig(), *layout_arena({"w": torch.ones(4)}, "cpu"))
    with pytest.raises(RuntimeError):
        m._ensure_plan(1, 8, 8)
    assert not any(c[0] == "plan" for c in fake.calls) and m._engines["movq"].plan_key is None


class _Recorder:
    """stands in for a class: records the keyword arguments of every construction"""

    def __init__(self):
        self.kw = []

    def __call__(self, *a, **kw):
        self.kw.append(kw)
        return self

    def load_state_dict(self, *a, **kw):
        return self

    def to(self, *a, **kw):
        return self

    def eval(self):
        return self


def test_movq_attention_passes_through_the_2_1_pipeline(monkeypatch, tmp_path):
    dec, enc = _Recorder(), _Recorder()
    monkeypatch.setattr(pipeline, "MoVQDecoderHIP", dec)
    monkeypatch.setattr(pipeline, "MoVQEncoderHIP", enc)
    mv = pipeline._MoVQ({"ddconfig": {}}, {}, torch.float16, "cpu", movq_attention="fused")
    mv.encoder
    assert dec.kw[0]["attention"] == "fused" and enc.kw[0]["attention"] == "fused"
    assert pipeline._MoVQ({"ddconfig": {}}, {}, torch.float16, "cpu").decoder.kw[-1]["attention"] == "auto"
    # get_kandinsky2 hands it to Kandinsky2_1HIP / Kandinsky2_2HIP
    for n in ("decoder_fp16.ckpt", "prior_fp16.ckpt", "movq_final.ckpt", "ViT-L-14_stats.th"):
        (tmp_path / n).write_bytes(b"")
    k21, k22 = _Recorder(), _Recorder()
    monkeypatch.setattr(pipeline, "Kandinsky2_1HIP", k21)
    monkeypatch.setattr(pipeline22, "Kandinsky2_2HIP", k22)
    pipeline.get_kandinsky2("cuda", cache_dir=str(tmp_path), conditioner=object(), movq_attention="scores")
    pipeline.get_kandinsky2("cuda", cache_dir=str(tmp_path), conditioner=object(), model_version="2.2", movq_attention="fused")
    pipeline.get_kandinsky2("cuda", cache_dir=str(tmp_path), conditioner=object())
    assert k21.kw[0]["movq_attention"] == "scores" and k22.kw[0]["movq_attention"] == "fused" and k21.kw[1]["movq_attention"] == "auto"


@pytest.mark.parametrize("task", ["text2img", "img2img"])
def test_movq_attention_passes_through_the_2_2_pipeline(monkeypatch, task):
    dec, enc, other = _Recorder(), _Recorder(), _Recorder()
    monkeypatch.setattr(pipeline22, "MoVQDecoderHIP", dec)
    monkeypatch.setattr(pipeline22, "MoVQEncoderHIP", enc)
    for name in ("UNet2DConditionHIP", "KandinskyV22DecoderHIP", "KandinskyV22Img2ImgDecoderHIP", "KandinskyV22InpaintDecoderHIP"):
        monkeypatch.setattr(pipeline22, name, other)
    arch = type("Arch", (), {"inpainting": False, "in_channels": 4})()
    monkeypatch.setattr(pipeline22, "make_arch22", lambda *a, **kw: arch)
    pipeline22.Kandinsky2_2HIP("cpu", task, unet_state_dict={}, movq_state_dict={}, conditioner=object(), movq_attention="fused")
    assert dec.kw[0]["attention"] == "fused"
    if task == "img2img":
        assert enc.kw[0]["attention"] == "fused"
    pipeline22.Kandinsky2_2HIP("cpu", task, unet_state_dict={}, movq_state_dict={}, conditioner=object())
    assert dec.kw[1]["attention"] == "auto"


def test_load_decoder22_hands_movq_attention_through_under_its_own_key(tmp_path):
    root = tmp_path / "kandinsky-2-2-decoder"
    for sub in ("unet", "movq", "scheduler"):
        (root / sub).mkdir(parents=True)
    torch.save({}, root / "unet" / "diffusion_pytorch_model.bin")
    torch.save({}, root / "movq" / "diffusion_pytorch_model.bin")
    assert pipeline22.load_decoder22_from_cache_dir(str(tmp_path), movq_attention="fused")["movq_attention"] == "fused"
    assert pipeline22.load_decoder22_from_cache_dir(str(tmp_path))["movq_attention"] == "auto"
