"""include/tfk.h read as text (no compiler): every ``ret tfk_name(params);`` prototype and every ``typedef struct`` body,
each parameter / field reduced to its class at the C-ABI -- what a ctypes binding has to get right:

    "ptr:<struct>"  pointer to one of the header's named structs      "ptr"  any other pointer
    "i32"  int32_t / int        "i64"  int64_t        "f32"  float        "struct:<name>"  a struct held by value (fields only)

Shared by tests/test_cabi_host.py (the binding table against the header) and tests/test_gpu_abi_calls.py (which entry
points take a stream, which arguments are pointers)."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfk.h")
_SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "float": "f32"}
_STRUCT_RE = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)


def _text() -> str:
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def struct_names():
    return [m.group(1) for m in _STRUCT_RE.finditer(_text())]


def _classify(type_words: str, pointer: bool, structs) -> str:
    words = [w for w in type_words.split() if w != "const"]
    if len(words) != 1:
        raise ValueError(f"cannot read the type {type_words!r}")
    if words[0] in structs:
        return ("ptr:" if pointer else "struct:") + words[0]
    if pointer:
        return "ptr"
    return _SCALARS[words[0]]            # KeyError: a scalar type this reader does not know -- extend it, do not guess


def _declarator(decl: str, structs):
    """'const float *x' -> ('ptr', 'x', None);  'float bn_eps[3]' -> ('f32', 'bn_eps', 3)."""
    m = re.fullmatch(r"\s*(.*?)(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", decl, flags=re.S)
    if m is None:
        raise ValueError(f"cannot read the declaration {decl!r}")
    return m.group(1), bool(m.group(2)), m.group(3), (int(m.group(4)) if m.group(4) else None)


def prototypes():
    """{name: (return class, [(class, parameter name), ...])} in the header's order."""
    structs = struct_names()
    text = _STRUCT_RE.sub("", _text())
    text = re.sub(r"enum\s*\{.*?\}\s*;", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"([\w \t\*]+?)\b(tfk_\w+)\s*\(([^)]*)\)\s*;", text):
        ret_words, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        ret = _classify(ret_words.replace("*", " "), "*" in ret_words, structs)
        plist = []
        if params != "void":
            for p in params.split(","):
                words, pointer, pname, count = _declarator(p, structs)
                if count is not None:
                    raise ValueError(f"{name}: array parameter {p!r}")
                plist.append((_classify(words, pointer, structs), pname))
        if name in out:
            raise ValueError(f"{name} is declared twice")
        out[name] = (ret, plist)
    return out


def structs():
    """{struct name: [(class, field name, array length or None), ...]} in declaration order."""
    names = struct_names()
    out = {}
    for m in _STRUCT_RE.finditer(_text()):
        fields = []
        for stmt in m.group(2).split(";"):
            if not stmt.strip():
                continue
            first, *rest = stmt.split(",")
            words, pointer, fname, count = _declarator(first, names)
            fields.append((_classify(words, pointer, names), fname, count))
            for r in rest:                    # 'const float *a, *b, c[3]': the later declarators share the type words
                _, pointer, fname, count = _declarator(r, names)
                fields.append((_classify(words, pointer, names), fname, count))
        out[m.group(1)] = fields
    return out


def takes_stream(proto) -> bool:
    """Does the entry point enqueue work (its prototype ends in ``void *stream``)?"""
    params = proto[1]
    return bool(params) and params[-1] == ("ptr", "stream")
