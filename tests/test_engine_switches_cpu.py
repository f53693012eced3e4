"""The switch table of INTEGRATION.md section G cannot drift from the sources, nor from the tests.

1. Every environment variable the package reads (env_flag(...), getenv(...), os.environ in kandinsky-2_amd/**) is named in the table, or in
   the developer-only list below with its reason.
2. Every switch of the table's first column is set by a test: by an item of tests/test_engine_switches_gpu.py (its SWITCHES tuple, and a
   monkeypatch that sets it there) or by the existing test file named below."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kandinsky-2_amd")
TESTS = os.path.join(ROOT, "tests")

# read by the sources, deliberately not in the user-facing table: one line of reason each
DEVELOPER_ONLY = {
    "K22_X2_OWN_LINES": "tools/make_tile_table.py --x2-only: no x3 fall-back, so that the asymmetric split's own table lines get measured",
    "K22_PRIOR_QKV_SPLIT": "split-K of the skinny c_qkv, measurement knob (profiles/r06_skinny.txt: 1 is the measured best and the default)",
    "K22_SKINNY_CFG": 'skinny.hip: "mt,nb" measurement override of the fixed tile rule',
    "K22_DBG_LDS_PAD": "tools/lds_victim_probe.py: LDS padding of the two-stream probe",
    "K22_LIB_PATH": "_lib.py: another build of the library (A/B of two builds)",
    "K22_IGEMM_STAGES": "default LDS-DMA ring depth of the generic kernel; the tile table's `stages` column is the supported way to set it",
}
# variables of other software that the package sets or reads for its own plumbing (parallel.py: torchrun's and the HSA runtime's)
NOT_OURS = re.compile(r"^(RANK|LOCAL_RANK|WORLD_SIZE|LOCAL_WORLD_SIZE|MASTER_ADDR|MASTER_PORT|HSA_[A-Z_]+)$")

# switch of the table's first column -> (test file that sets it, the text that file must hold).  The default text is a
# monkeypatch.setenv("<switch>", ...) call.
GPU_FILE = "test_engine_switches_gpu.py"
SWITCH_TESTS = {
    "K22_AUTOTUNE": ("test_up2_phase_gpu.py", None),
    "K22_STREAM": (GPU_FILE, None),
    "K22_FUSE_SKIP": (GPU_FILE, None),
    "K22_X2_PLAN": (GPU_FILE, None),
    "K22_PRIOR_SKINNY": (GPU_FILE, None),
    "K22_CHAINS": ("test_unet22_gpu.py", None),
    "K22_UP_PHASE": ("test_up2_phase_gpu.py", None),
    "K22_HOIST_TIME": ("test_sampler_loop_gpu.py", None),
    # a launcher-level static, read once per process: tested through its in-process form, the table's next row
    "K22_ATT_PIPE": ("test_attention_parity_gpu.py", 'b"att_pipe"'),
    # read once, when the library is opened (_lib.lib()): what it does is k22_tile_table_load, which these files drive directly
    "K22_TILE_TABLE": (GPU_FILE, "k22_tile_table_load"),
}


def _section_g():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    start = text.index("\n## G. ")
    end = text.find("\n## ", start + 1)
    return text[start:end if end > 0 else len(text)]


def _table_rows():
    """the rows of the ONE table that starts at the `| variable | default | effect |` header: a blank line ends a Markdown table"""
    lines = _section_g().splitlines()
    at = next(i for i, ln in enumerate(lines) if re.match(r"^\|\s*variable\s*\|\s*default\s*\|\s*effect\s*\|\s*$", ln))
    assert re.match(r"^\|(\s*-+\s*\|)+\s*$", lines[at + 1]), lines[at + 1]
    rows = []
    for ln in lines[at + 2:]:
        if not ln.startswith("|"):
            break
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        assert len(cells) == 3, f"a table row with {len(cells)} cells: {ln[:80]}"
        rows.append(cells)
    return rows


def documented_names():
    """every K22_* name anywhere in the table's rows"""
    return {n for cells in _table_rows() for c in cells for n in re.findall(r"\bK22_[A-Z0-9_]+\b", c)}


def table_switches():
    """the environment switches the table's first column sets"""
    return [n for cells in _table_rows() for n in re.findall(r"\bK22_[A-Z0-9_]+\b", cells[0])]


def names_read_by_the_sources():
    found = {}
    pats = [re.compile(r'\benv_flag\(\s*"([A-Za-z0-9_]+)"'), re.compile(r'\bgetenv\(\s*"([A-Za-z0-9_]+)"'),
            re.compile(r'os\.environ(?:\.get|\.setdefault|\.pop)?[\[(]\s*"([A-Za-z0-9_]+)"'),
            re.compile(r'"([A-Za-z0-9_]+)"\s+(?:not\s+)?in\s+os\.environ')]
    for d, _dirs, files in os.walk(PKG):
        for fn in files:
            if not fn.endswith((".hip", ".h", ".py")):
                continue
            path = os.path.join(d, fn)
            with open(path, errors="replace") as f:
                text = f.read()
            for p in pats:
                for m in p.finditer(text):
                    found.setdefault(m.group(1), set()).add(os.path.relpath(path, ROOT))
    return found


def test_the_parsers_see_what_is_there():
    """the sweep below is only as good as its two readers: each must find names that are known to exist"""
    read = names_read_by_the_sources()
    for n in ("K22_FUSE_SKIP", "K22_PRIOR_SKINNY", "K22_X2_PLAN", "K22_TUNE_CACHE", "K22_TILE_TABLE", "K22_CHAINS", "K22_LIB_PATH", "K22_ATT_PIPE"):
        assert n in read, n
    assert len(_table_rows()) >= 11 and table_switches()[0] == "K22_TILE_TABLE"


def test_every_variable_the_sources_read_is_documented_or_listed_as_developer_only():
    read, doc = names_read_by_the_sources(), documented_names()
    ours = {n: w for n, w in read.items() if not NOT_OURS.match(n)}
    assert all(n.startswith("K22_") for n in ours), sorted(n for n in ours if not n.startswith("K22_"))
    missing = {n: sorted(w) for n, w in ours.items() if n not in doc and n not in DEVELOPER_ONLY}
    assert not missing, f"read by the sources, neither in INTEGRATION.md section G's table nor in DEVELOPER_ONLY: {missing}"
    assert not set(DEVELOPER_ONLY) & doc, f"documented AND listed as developer-only: {sorted(set(DEVELOPER_ONLY) & doc)}"
    stale = sorted(n for n in DEVELOPER_ONLY if n not in read)
    assert not stale, f"listed as developer-only but no longer read: {stale}"
    gone = sorted(n for n in table_switches() if n not in read)
    assert not gone, f"a switch of the table that no source reads: {gone}"


def test_every_documented_switch_is_set_by_a_test():
    switches = table_switches()
    assert len(set(switches)) == len(switches)
    assert set(SWITCH_TESTS) == set(switches), (sorted(set(switches) - set(SWITCH_TESTS)), sorted(set(SWITCH_TESTS) - set(switches)))
    with open(os.path.join(TESTS, GPU_FILE)) as f:
        gpu_text = f.read()
    owned = re.search(r"^SWITCHES = \(([^)]*)\)", gpu_text, re.M)
    owned = set(re.findall(r'"(K22_[A-Z0-9_]+)"', owned.group(1)))
    assert owned == {s for s, (fn, text) in SWITCH_TESTS.items() if fn == GPU_FILE and text is None}
    for s in sorted(owned):
        # set through _env(mp, K22_X=...) or _env(mp, **{"K22_X": ...}) by at least one item
        assert re.search(r"_env\([^)\n]*\b%s=" % s, gpu_text) or re.search(r'_env\([^\n]*"%s":' % s, gpu_text), f"{GPU_FILE} never sets {s}"
    for s, (fn, text) in SWITCH_TESTS.items():
        with open(os.path.join(TESTS, fn)) as f:
            body = f.read()
        if fn == GPU_FILE and text is None:
            continue
        want = text or 'monkeypatch.setenv("%s"' % s
        assert want in body, f"tests/{fn} does not hold {want!r} ({s})"
