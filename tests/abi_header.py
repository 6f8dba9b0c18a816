"""include/cvlm.h read as data: what the ctypes binding (camouflaged_vlm_amd/hip.py) is held against in tests/test_host_cpu.py.

The header is regular: prototypes `int | int64_t | const char* cvlm_x(...);`, parameters that are pointers, int, int32_t, int64_t or
float, two flat `typedef struct`s and one (cvlm_gemm_plan_info) with a nested anonymous struct array.  C types come back as strings
with single spaces and the `*` attached ("const float*", "int32_t", "char[128]"); anything outside that grammar raises."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvlm.h")


def _code(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _decl(decl: str):
    """'const float* x' -> ('const float*', 'x'); 'char kernel[128]' -> ('char[128]', 'kernel')."""
    m = re.fullmatch(r"\s*((?:const\s+)?\w+)\s*(\*?)\s*(\w+)\s*((?:\[\d+\])?)\s*", decl)
    assert m, f"unexpected declaration {decl!r}"
    return " ".join(m.group(1).split()) + m.group(2) + m.group(4), m.group(3)


def prototypes(text: str = None) -> dict:
    """name -> (return type, [(parameter type, parameter name), ...]) for every function the header declares, in its order."""
    code = _code(open(HEADER).read() if text is None else text)
    out = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(cvlm_\w+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        params = params.strip()
        out[name] = (ret.replace(" *", "*").strip(), [] if params == "void" else [_decl(p) for p in params.split(",")])
    return out


def _fields(body: str) -> list:
    """Fields of a struct body in order: (C type, name), or ('struct[n]', name, fields of the nested struct)."""
    out = []
    while body.strip():
        m = re.match(r"\s*struct\s*\{(.*?)\}\s*(\w+)\s*\[(\d+)\]\s*;", body, flags=re.S)
        if m:
            out.append((f"struct[{m.group(3)}]", m.group(2), _fields(m.group(1))))
        else:
            m = re.match(r"\s*([^;{}]+);", body)
            assert m, f"unexpected struct text {body[:60]!r}"
            first, *more = m.group(1).split(",")
            ctype, name = _decl(first)                           # `int32_t M, N, K, batch;`: the type of the first holds for all
            assert not more or not ctype.endswith(("*", "]")), m.group(1)
            out += [(ctype, name)] + [(ctype, n.strip()) for n in more]
        body = body[m.end():]
    return out


def structs(text: str = None) -> dict:
    """typedef name -> fields (see _fields) for every `typedef struct` of the header."""
    code = _code(open(HEADER).read() if text is None else text)
    return {name: _fields(body) for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\n\} \1;", code, flags=re.S)}
