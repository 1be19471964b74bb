"""Loading libbfhip.so and calling into it: the two library handles, the errors, and the marshalling every module of the mirror shares.
What the C ABI declares (prototypes, struct layouts, constants) is _abi_gen.py, generated from include/bfhip.h."""
import ctypes
import os

from . import _abi_gen
from ._abi_gen import BFHIP_TRACE_REJECTED as TRACE_REJECTED

_HERE = os.path.dirname(os.path.abspath(__file__))
# BFHIP_LIBRARY: another build of the library (A/B runs; tests of the late-host and RCCL-double paths name libbfhip_testhooks.so, the
# -DBFHIP_TEST_HOOKS build — the default library has no test hooks)
_LIB_PATH = os.environ.get("BFHIP_LIBRARY") or os.path.join(_HERE, "libbfhip.so")
TESTHOOKS_LIBRARY = os.path.join(_HERE, "libbfhip_testhooks.so")
_lib = None
_abi = None

P = (1 << 31) - 1


class BfhipError(RuntimeError):
    pass


def lib():
    """Load libbfhip.so (built in-tree by `make -C stwo-brainfuck_amd/csrc`). Fails loudly when it is missing. The RAW handle: no
    prototypes, for callers with calling conventions of their own (tests, tools). The package itself calls through abi()."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise BfhipError(f"{_LIB_PATH} is missing: build it with __graft_entry__.build(); there is no CPU fallback")
        _lib = ctypes.CDLL(_LIB_PATH)
        _lib.bfhip_last_error.restype = ctypes.c_char_p
    return _lib


class _TypedLibrary(ctypes.CDLL):
    """A handle of its own (its function objects are not lib()'s) on which every function has the header's prototype, set when the
    function is first looked up. ctypes then passes each scalar at its declared width and refuses a call of the wrong arity."""

    def __getitem__(self, name):
        func = super().__getitem__(name)
        func.restype, func.argtypes = _abi_gen.FUNCTIONS[name]
        return func


def abi():
    """The typed handle of the same library: what every call inside the package goes through."""
    global _abi
    if _abi is None:
        lib()
        _abi = _TypedLibrary(_LIB_PATH)
    return _abi


class TraceRejected(BfhipError):
    """BFHIP_TRACE_REJECTED: a proof's preflight (Context.set_preflight) refused the trace before proving it. str() = the rejection lines
    (bfhip_format_preflight); .check = the CheckResult of the 13 components, .relations = the RelationResult of the tuples that do not
    cancel (empty unless the logUp total is not zero)."""

    def __init__(self, text, check=None, relations=None):
        super().__init__(text)
        self.check, self.relations = check, relations


def _last_error():
    return BfhipError(abi().bfhip_last_error().decode())


def _check(rc):
    if rc != 0:
        raise _last_error()


def _check_proof(rc, ctx):
    """_check for the proving entry points: BFHIP_TRACE_REJECTED raises TraceRejected with the context's preflight report."""
    if rc == TRACE_REJECTED:
        text = abi().bfhip_last_error().decode()
        raise TraceRejected(text, *ctx.last_preflight())
    _check(rc)


def struct_fields(c_name, **nested):
    """_fields_ of a by-value struct of include/bfhip.h. nested: the mirror's own class for each struct it embeds, so that what an
    embedded array hands out carries that class's methods."""
    return [(n, nested[t[0]] * t[1] if isinstance(t, tuple) else t) for n, t in _abi_gen.STRUCTS[c_name]]


def _u32s(values):
    values = [int(v) for v in values]
    return (ctypes.c_uint32 * len(values))(*values)


def _ptr_array(ptrs):
    """A host array of device pointers; None or 0 is a null entry."""
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _qm31s(values, what):
    """(the words flat as a u32 array or None if there are none, the count) of QM31 values of 4 words each."""
    values = [list(q) for q in values]
    if any(len(q) != 4 for q in values):
        raise ValueError(what + " is 4 words")
    return _u32s([w for q in values for w in q]) if values else None, len(values)


def _take_host_string(ptr, n=None):
    """The bytes of a malloc'd result (n bytes, or up to its NUL), freed with bfhip_free_host."""
    data = ctypes.string_at(ptr, -1 if n is None else n)
    abi().bfhip_free_host(ptr)
    return data


def _two_pass_text(entry, *args):
    """An entry that writes text into (buffer, capacity, *needed): asked for the size (rc -2 = too small is expected), then for the text."""
    need = ctypes.c_size_t()
    if entry(*args, None, 0, ctypes.byref(need)) not in (0, -2):
        raise _last_error()
    buf = ctypes.create_string_buffer(need.value)
    _check(entry(*args, buf, need.value, None))
    return buf.value.decode()


class Owned:
    """An object that owns one handle of the library, self._h: close() hands it to the class's destroy entry once; the object is a
    context manager, and unless _close_on_del is False it also closes when it is collected."""
    _destroy = None
    _close_on_del = True

    def close(self):
        if self._h:
            getattr(abi(), self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if self._close_on_del:
            try:
                self.close()
            except Exception:
                pass
