"""The one reader of include/bfhip.h: what the C ABI declares, for the generators of its mirrors (tools/gen_rust_ffi.py ->
bindings/rust/bfhip_sys.rs, tools/gen_python_abi.py -> stwo-brainfuck_amd/_abi_gen.py). Regular expressions over the header's own
plain style, not a C parser: one declarator per parameter, `T a, b[N];` fields, anonymous `enum { NAME = value, ... }` constants."""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfhip.h")

# ctype: the C type with every `*` attached and a parameter's `[N]` turned into one more `*`; array: N of a struct field `T name[N]`, else None
Param = collections.namedtuple("Param", "ctype name")
Field = collections.namedtuple("Field", "ctype name array")
Function = collections.namedtuple("Function", "ret name params")
# typedefs: (name, fields) in header order, fields None for an opaque handle (`typedef struct X X;`); constants: (NAME, value) in header order
Header = collections.namedtuple("Header", "functions typedefs constants")


def _ctype(text):
    return re.sub(r"\s*\*\s*", "*", " ".join(text.split()))


def _fields(body):
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"^(.*?[\s*])(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)$", decl, flags=re.S)
        for name in m.group(2).split(","):
            n = re.match(r"^\s*(\w+)(?:\[(\d+)\])?$", name)
            out.append(Field(_ctype(m.group(1)), n.group(1), int(n.group(2)) if n.group(2) else None))
    return out


def parse(text=None):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read() if text is None else text, flags=re.S)
    functions = []
    for ret, name, params in re.findall(r"^(const char\*|int32_t|void)\s+(bfhip_\w+)\s*\((.*?)\)\s*;", text, flags=re.S | re.M):
        args = []
        for p in filter(lambda p: p and p != "void", (" ".join(p.split()) for p in params.split(","))):
            m = re.match(r"^(.*?)(\w+)(\[\d*\])?$", p)
            args.append(Param(_ctype(m.group(1)) + ("*" if m.group(3) else ""), m.group(2)))
        functions.append(Function(ret, name, args))
    typedefs = [(m.group(1), None if m.group(2) is None else _fields(m.group(2)))
                for m in re.finditer(r"^typedef struct (\w+)\s*(?:\{(.*?)\}\s*)?\1;", text, flags=re.S | re.M)]
    constants = [(name, int(value)) for body in re.findall(r"^enum\s*\{(.*?)\}\s*;", text, flags=re.S | re.M)
                 for name, value in re.findall(r"(\w+)\s*=\s*(-?\d+)", body)]
    return Header(functions, typedefs, constants)
