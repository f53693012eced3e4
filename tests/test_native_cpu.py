"""kandinsky2_amd.native on the host: the arena layout, and the engine handle / module base driven with four recording callables in place of
the C entries (device "cpu": no GPU, and no native code is run)."""
import pytest
import torch

from kandinsky2_amd import _lib
from kandinsky2_amd.native import NativeEngine, NativeModule, arena_size, layout_arena


class FakeEntries:
    """create / destroy / plan / bind of a made-up family; `fail_plans` plan calls return an error code first"""

    def __init__(self, ws_bytes=1000, fail_plans=0):
        self.calls, self.ws_bytes, self.fail_plans = [], ws_bytes, fail_plans

    def create(self, cfg, weights, n, handle):
        self.calls.append(("create", n, [(weights[i].name, weights[i].ptr) for i in range(n)]))
        handle._obj.value = 0x1000
        return 0

    def destroy(self, handle):
        self.calls.append(("destroy", handle.value))

    def plan(self, handle, *shape_and_size):
        *shape, size = shape_and_size
        self.calls.append(("plan", tuple(shape)))
        if self.fail_plans:
            self.fail_plans -= 1
            return -1
        size._obj.value = self.ws_bytes
        return 0

    def bind(self, handle, ptr, nbytes):
        self.calls.append(("bind", ptr, nbytes))
        return 0

    def family(self):
        return self.create, self.destroy, self.plan, self.bind

    def count(self, what):
        return sum(c[0] == what for c in self.calls)


def _engine(fake):
    arena, table = layout_arena({"a": torch.ones(3), "b": torch.ones(70, dtype=torch.bfloat16)}, "cpu")
    return NativeEngine(fake.family(), _lib.K22PriorConfig(), arena, table), arena, table


def test_layout_arena_offsets_size_padding_and_meta_table():
    g = torch.Generator().manual_seed(0)
    ent = {"w": torch.randn(5, 13, generator=g), "b": torch.randn(64, generator=g).to(torch.bfloat16), "x": torch.randn(1, generator=g),
           "h": torch.randn(300, generator=g).to(torch.float16)}
    arena, table = layout_arena(ent, "cpu")
    assert list(table) == list(ent) and arena.dtype == torch.uint8
    assert [n for _o, n in table.values()] == [260, 128, 4, 600]
    assert all(o % 256 == 0 for o, _n in table.values()) and [o for o, _n in table.values()] == [0, 512, 768, 1024]
    last_off, last_n = table["h"]
    assert arena.numel() == last_off + (last_n + 255) // 256 * 256 + 256 == arena_size(table) == 2048
    covered = torch.zeros(arena.numel(), dtype=torch.bool)
    for name, (o, n) in table.items():
        assert torch.equal(arena[o:o + n], ent[name].reshape(-1).view(torch.uint8))
        covered[o:o + n] = True
    assert not arena[~covered].any()                                   # bytes outside the entries are zero
    meta, meta_table = layout_arena({k: torch.empty(v.shape, dtype=v.dtype, device="meta") for k, v in ent.items()}, "meta")
    assert meta.is_meta and meta.numel() == arena.numel() and meta_table == table


def test_engine_passes_the_arena_pointers_and_plans_once_per_key():
    fake = FakeEntries()
    e, arena, table = _engine(fake)
    assert fake.calls == [("create", 2, [(b"a", arena.data_ptr()), (b"b", arena.data_ptr() + 256)])]
    assert e.handle.value == 0x1000 and e.plan_key is None and e.ws is None
    e.ensure_plan(2, 16, 16)
    e.ensure_plan(2, 16, 16)
    assert fake.count("plan") == fake.count("bind") == 1 and e.plan_key == (2, 16, 16)
    _, ptr, nbytes = fake.calls[-1]
    lo = e.ws.data_ptr()
    assert nbytes == 1000 and ptr % 256 == 0 and lo <= ptr and ptr + nbytes <= lo + e.ws.numel()      # aligned and inside the workspace
    e.ensure_plan(4, 16, 16)
    assert [c for c in fake.calls if c[0] == "plan"] == [("plan", (2, 16, 16)), ("plan", (4, 16, 16))] and e.plan_key == (4, 16, 16)
    e.ensure_plan(2, 16, 16)                                           # back to the first key: a plan of its own again
    assert fake.count("plan") == fake.count("bind") == 3


def test_a_failed_plan_leaves_no_plan_key_and_the_next_call_plans_again():
    fake = FakeEntries()
    e, _arena, _table = _engine(fake)
    e.ensure_plan(1)
    assert e.plan_key == (1,)
    fake.fail_plans = 1
    with pytest.raises(RuntimeError):
        e.ensure_plan(2)
    assert e.plan_key is None and fake.count("bind") == 1
    e.ensure_plan(1)                                                   # the key of the last finished plan: planned again all the same
    assert e.plan_key == (1,) and fake.count("plan") == 3 and fake.count("bind") == 2


def test_close_twice_destroys_once_and_del_after_close_destroys_nothing():
    fake = FakeEntries()
    e, _arena, _table = _engine(fake)
    e.ensure_plan(1)
    e.close()
    e.close()
    assert fake.count("destroy") == 1 and e.handle is None and e.arena is None and e.ws is None and e.plan_key is None
    e.__del__()
    del e
    assert fake.count("destroy") == 1
    e2, _arena, _table = _engine(fake)
    del e2                                                             # never closed: __del__ destroys
    assert fake.count("destroy") == 2


class TwoParams(NativeModule):
    def __init__(self, fake):
        super().__init__({"lin.weight": (4, 3), "lin.bias": (4,)}, torch.bfloat16)
        self.fake, self.released = fake, 0

    def build(self):
        arena, table = layout_arena({k: v.detach() for k, v in self.state_dict().items()}, "cpu")
        self._engines["only"] = NativeEngine(self.fake.family(), _lib.K22PriorConfig(), arena, table)
        return self._engines["only"]

    def _release(self):
        super()._release()
        self.released += 1


def test_module_base_releases_its_engines_on_load_state_dict_and_on_apply():
    fake = FakeEntries()
    m = TwoParams(fake)
    assert list(m.state_dict()) == ["lin.weight", "lin.bias"] and m._handle is None and m._arena is None and m._ws is None
    e = m.build()
    e.ensure_plan(3)
    assert m._handle is e.handle and m._arena is e.arena and m._ws is e.ws
    m.load_state_dict({"lin.weight": torch.ones(4, 3), "lin.bias": torch.ones(4)})
    assert m.released == 1 and fake.count("destroy") == 1 and not m._engines and m._handle is None and m._ws is None and e.handle is None
    assert float(m.lin.weight.sum()) == 12.0
    m.build()
    m.double()                                                         # any _apply: a device move, a cast
    assert m.released == 2 and fake.count("destroy") == 2 and not m._engines
    m.build()
    m.__del__()
    assert fake.count("destroy") == 3
    with pytest.raises(RuntimeError, match=r"TwoParams runs on the GPU only \(no CPU fallback\)"):
        m._device()
