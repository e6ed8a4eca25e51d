"""The prototypes of include/dddmr_rollout.h as kinds: what tests/test_capi_cpu.py compares with _capi.SIGNATURES and
what tools/binding_trace.py reads to tell a pointer from a number."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include", "dddmr_rollout.h")

_SCALARS = {"size_t": "size_t", "int": "int", "int32_t": "int", "uint32_t": "uint32", "int64_t": "int64", "double": "double"}


def _kind(decl: str, is_return: bool = False) -> str:
    """'const float* xyz' -> 'in' (a pointer or array to const), 'float out[4]' -> 'out', 'size_t n' -> 'size_t', ..."""
    words = re.findall(r"\w+", decl)
    if "*" in decl or "[" in decl:
        if is_return:
            assert words == ["const", "char"], decl
            return "str"
        return "in" if words[0] == "const" else "out"
    words = [w for w in words if w != "const"]
    base = words[0] if is_return or len(words) == 1 else words[-2]     # (a parameter's last word is its name)
    return "void" if base == "void" else _SCALARS[base]


def prototypes(path: str = HEADER) -> dict:
    """name -> (return kind, [parameter kinds]) for every dddmr_rollout_* function the header declares."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\b(dddmr_rollout_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        if params == ["void"] or params == [""]:
            params = []
        assert name not in out, name
        out[name] = (_kind(ret.strip(), True), [_kind(p) for p in params])
    return out


def ctypes_kind(t, is_return: bool = False) -> str:
    """The same kinds for a ctypes type; a pointer is 'ptr' whatever it points to (ctypes has no const)."""
    if t is None:
        return "void"
    if t is C.c_char_p and is_return:
        return "str"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    return {C.c_size_t: "size_t", C.c_int32: "int", C.c_uint32: "uint32", C.c_int64: "int64", C.c_double: "double"}[t]
