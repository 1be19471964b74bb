"""CPU: the Python mirror takes what it knows of the C ABI from include/bfhip.h. The generated files are in step with the header, every
declared function has a prototype of the right arity and widths, the package calls through the typed handle while lib() stays raw, and
the names the package showed before it was split into modules are all still there."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from test_abi_and_replicas import declared_symbols

PKG_DIR = os.path.join(ROOT, "stwo-brainfuck_amd")


def _header_prototypes():
    """{function: [parameter declarations]} read from the header text here, independently of tools/bfhip_header.py."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bfhip.h")).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(bfhip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        out[name] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return out


@pytest.fixture(scope="module")
def abi_gen(pkg):
    return sys.modules[pkg.__name__ + "._abi_gen"]


@pytest.fixture(scope="module")
def typed(pkg):
    return sys.modules[pkg.__name__ + "._abi"].abi()


def test_generated_files_are_in_step_with_the_header():
    """Running the two generators reproduces the committed _abi_gen.py and bfhip_sys.rs byte for byte."""
    paths = [os.path.join(PKG_DIR, "_abi_gen.py"), os.path.join(ROOT, "bindings", "rust", "bfhip_sys.rs")]
    committed = [open(p, "rb").read() for p in paths]
    try:
        for tool in ("gen_python_abi.py", "gen_rust_ffi.py"):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
        fresh = [open(p, "rb").read() for p in paths]
    finally:
        for p, data in zip(paths, committed):
            open(p, "wb").write(data)
    assert fresh[0] == committed[0], "_abi_gen.py is stale: run tools/gen_python_abi.py"
    assert fresh[1] == committed[1], "bfhip_sys.rs is stale: run tools/gen_rust_ffi.py"


def test_every_declared_symbol_has_a_prototype_of_the_headers_arity(abi_gen):
    protos = _header_prototypes()
    syms = declared_symbols()
    assert len(syms) >= 91 and sorted(protos) == syms == sorted(abi_gen.FUNCTIONS)
    for name in syms:
        restype, argtypes = abi_gen.FUNCTIONS[name]
        assert len(argtypes) == len(protos[name]), (name, argtypes, protos[name])


def test_64_bit_scalars_are_64_bit_in_the_prototypes(abi_gen):
    """Every by-value uint64_t, size_t or double parameter of the header is an 8-byte ctypes type of its kind; every other by-value
    scalar is narrower, every pointer (arrays included) a c_void_p."""
    kinds = {"uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    seen = dict.fromkeys(kinds, 0)
    for name, params in _header_prototypes().items():
        argtypes = abi_gen.FUNCTIONS[name][1]
        for k, decl in enumerate(params):
            if "*" in decl or "[" in decl:
                assert argtypes[k] is ctypes.c_void_p, (name, decl)
                continue
            ctype = decl.replace("const ", "").split()[0]
            if ctype in kinds:
                seen[ctype] += 1
                assert argtypes[k] is kinds[ctype] and ctypes.sizeof(argtypes[k]) == 8, (name, decl, argtypes[k])
            else:
                assert ctype in ("int32_t", "uint32_t", "uint8_t") and ctypes.sizeof(argtypes[k]) == {"uint8_t": 1}.get(ctype, 4), (name, decl, argtypes[k])
    assert all(seen.values()), seen      # at least one of each kind, or this test checks nothing


def test_structs_and_constants_come_from_the_header(pkg, abi_gen):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bfhip.h")).read(), flags=re.S)
    constants = {n: int(v) for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S) for n, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", body)}
    assert len(constants) >= 49
    for name, value in constants.items():
        assert getattr(abi_gen, name) == value
        if hasattr(pkg, name[len("BFHIP_"):]):
            assert getattr(pkg, name[len("BFHIP_"):]) == value
    for short in ("TRACE_REJECTED", "JOB_CANCELLED", "POOL_MAX_OUTSTANDING", "LOGUP_FRAC", "REL_WORD", "AIR_C_EXT", "AIR_MAX_OFFSET", "CHANNEL_POSEIDON252", "PCS_MAX_TREES"):
        assert getattr(pkg, short) == constants["BFHIP_" + short]
    assert sorted(abi_gen.STRUCTS) == sorted(re.findall(r"typedef struct (\w+)\s*\{", text))
    # an embedded struct is the mirror's own class, so that its elements carry the methods
    rep = pkg.PreflightReport()
    assert isinstance(rep.components[0], pkg.CheckReport) and isinstance(rep.relations[2], pkg.RelationReport) and isinstance(rep.entries[11], pkg.RelationEntry)
    assert rep.components[3].as_dict()["name"] == "memory" and ctypes.sizeof(rep) == 4064


def test_the_raw_handle_stays_raw_and_the_typed_one_checks_arity(pkg, typed):
    assert pkg.lib().bfhip_ctx_create.argtypes is None and pkg.lib().bfhip_channel_mix_u64.argtypes is None
    assert typed is not pkg.lib() and typed.bfhip_ctx_create is not pkg.lib().bfhip_ctx_create
    assert typed.bfhip_ctx_create.argtypes == [ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p]
    with pytest.raises(TypeError):
        typed.bfhip_ctx_create(0, 20)
    with pytest.raises(TypeError):
        typed.bfhip_channel_mix_u64(None)
    assert typed.bfhip_last_error.restype is ctypes.c_char_p and typed.bfhip_free_host.restype is None


def test_surface_is_a_superset_of_the_recorded_one(pkg):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        from make_python_surface import surface
    finally:
        sys.path.pop(0)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "python_surface.json")))
    have = surface(pkg)
    assert len(want["names"]) >= 128 and {"_check", "_LIB_PATH", "lib", "Context", "AirBuilder"} <= set(want["names"])
    assert set(want["names"]) <= set(have["names"]), sorted(set(want["names"]) - set(have["names"]))
    for cls, attrs in want["classes"].items():
        assert set(attrs) <= set(have["classes"][cls]), (cls, sorted(set(attrs) - set(have["classes"][cls])))
    assert os.path.samefile(os.path.dirname(pkg._LIB_PATH), PKG_DIR)
    with pytest.raises(pkg.BfhipError):
        pkg._check(-1)


@pytest.mark.parametrize("value", [(1 << 40) + 3, (1 << 31) - 5])
def test_u64_width_round_trip_on_a_host_only_entry(pkg, value):
    """Channel.mix_u64 through the typed handle reaches the state that the raw handle reaches with an explicit c_uint64."""
    ch = pkg.Channel()
    ch.mix_u64(value)
    L, h = pkg.lib(), ctypes.c_void_p()
    assert L.bfhip_channel_create(ctypes.byref(pkg.Conventions()), ctypes.byref(h)) == 0
    try:
        assert L.bfhip_channel_mix_u64(h, ctypes.c_uint64(value)) == 0
        d, n = (ctypes.c_uint8 * 32)(), ctypes.c_uint32()
        assert L.bfhip_channel_state(h, d, ctypes.byref(n)) == 0
        assert ch.state() == (bytes(d), n.value) and ch.state() != pkg.Channel().state()
        # the low word alone is another value: a call that dropped the high word would not reach this state
        low = pkg.Channel()
        low.mix_u64(value & 0xFFFFFFFF)
        assert (low.state() == ch.state()) == (value < 1 << 32)
    finally:
        L.bfhip_channel_destroy(h)
        ch.close()


def test_set_default_conventions_reaches_every_module(pkg):
    """The default is module state of context.py that pcs.py and prove.py read: a Channel made afterwards adopts it."""
    try:
        pkg.set_default_conventions(1, 1, 1, 0)
        assert pkg.Channel().conventions == (1, 1, 1, 0) and tuple(pkg._default_conventions) == (1, 1, 1, 0)
    finally:
        pkg.set_default_conventions(0, 0, 0, 0)
    assert pkg.Channel().conventions == (0, 0, 0, 0)


def test_the_old_calling_style_is_gone():
    """No call through the raw handle inside the package outside _abi.py, and no by-value ctypes wrap at a call site (the zero-argument
    out-parameter form stays). __init__.py holds imports only."""
    import ast
    modules = sorted(f for f in os.listdir(PKG_DIR) if f.endswith(".py"))
    assert {"__init__.py", "_abi.py", "_abi_gen.py"} <= set(modules)
    for f in modules:
        src = open(os.path.join(PKG_DIR, f)).read()
        if f != "_abi.py":
            assert "lib().bfhip_" not in src, f
        wraps = re.findall(r"ctypes\.c_(?:size_t|uint64|uint32|double|void_p)\([^)]", src)
        assert not wraps, (f, wraps)
    tree = ast.parse(open(os.path.join(PKG_DIR, "__init__.py")).read())
    assert all(isinstance(node, (ast.Import, ast.ImportFrom)) or (isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant)) for node in tree.body)
