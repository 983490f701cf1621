"""The C ABI of ``libsrlhip.so`` as ctypes, read from ``include/srl_hip.h``: the header ``csrc/*.hip`` is compiled against is
the only place a prototype, a struct layout or a constant is written down.  Host-only (no torch, no library, no device).

The parser accepts the header's own style and nothing else -- integer ``#define SRL_*``, ``enum { NAME [= int], ... }``,
``typedef struct srl_x { ... } srl_x;`` and prototypes ``ret srl_name(args);`` -- and raises ``CabiError`` on whatever is left
over, so a declaration it cannot read is an import error here, not wrong bytes in a kernel's arguments.

Type map: scalars to their ctypes; ``char*`` to ``c_char_p``; a pointer to a parsed struct to ``POINTER(<its Structure>)``;
every other pointer (``void**`` and ``const float* const*`` included) to ``c_void_p`` -- the header cannot tell a device
pointer from a host array, and ``c_void_p`` takes the addresses, ctypes arrays and ``byref()`` objects the wrappers pass.
"""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srl_hip.h")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
            "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float,
            "double": ctypes.c_double}
_POINTEE_ONLY = ("void", "char")
RENAMES = {"in": "in_"}  # struct fields whose C name is a Python keyword; every other field keeps the header's name


class CabiError(ValueError):
    pass


def parse(text):
    """``(consts, structs, prototypes)`` of a header: {name: int}, {name: Structure class}, {name: (restype, [argtypes])}."""
    consts, structs, prototypes = {}, {}, {}

    def integer(s, what):
        if re.fullmatch(r"-?(\d+|0[xX][0-9a-fA-F]+)", s):
            return int(s, 0)
        if s in consts:
            return consts[s]
        raise CabiError(f"{what}: {s!r} is neither an integer nor a constant defined above it")

    def ctype(decl, what):
        """C declaration ``[const] base [*...] [name]`` -> (ctypes type, name or None)."""
        toks = [t for t in decl.replace("*", " ").split() if t != "const"]
        if not 1 <= len(toks) <= 2:
            raise CabiError(f"{what}: cannot read the declaration {decl.strip()!r}")
        base, stars, name = toks[0], decl.count("*"), toks[1] if len(toks) == 2 else None
        if not (base in _SCALARS or base in structs or (stars and base in _POINTEE_ONLY)):
            raise CabiError(f"{what}: unknown type {base!r} in {decl.strip()!r}")
        if not stars:
            return (_SCALARS.get(base) or structs[base]), name
        if stars == 1 and base == "char":
            return ctypes.c_char_p, name
        if stars == 1 and base in structs:
            return ctypes.POINTER(structs[base]), name
        return ctypes.c_void_p, name

    def define(m):
        consts[m.group(1)] = integer(m.group(2), m.group(1))
        return ""

    def enum(m):
        value = -1
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            im = re.fullmatch(r"(\w+)(?:\s*=\s*(\S+))?", item)
            if not im:
                raise CabiError(f"enum: cannot read the enumerator {item!r}")
            value = consts[im.group(1)] = value + 1 if im.group(2) is None else integer(im.group(2), im.group(1))
        return ""

    def struct(m):
        tag, body, name = m.groups()
        if tag != name:
            raise CabiError(f"typedef struct {tag}: the typedef's name {name!r} differs from the tag")
        fields = []
        for decl in filter(None, (s.strip() for s in body.split(";"))):
            # `int64_t ld_self, ld_key[SRL_EATTN_MAX_KEYS], ld_mask;` / `float *g_emb, *g_w_ih;`: a `*` belongs to its declarator
            base, rest = re.fullmatch(r"((?:const\s+)?\w+)(.*)", decl, re.S).groups()
            for d in rest.split(","):
                dm = re.fullmatch(r"\s*([*\s]*\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", d)
                if not dm:
                    raise CabiError(f"{name}: cannot read the field {d.strip()!r} of {decl!r}")
                t, field = ctype(f"{base} {dm.group(1)}", name)
                if dm.group(2) is not None:
                    t = t * integer(dm.group(2), f"{name}.{field}: array extent")
                fields.append((RENAMES.get(field, field), t))
        cls_name = "".join(w.capitalize() for w in name.split("_")[1:])  # srl_ppo_hparams -> PpoHparams
        structs[name] = type(cls_name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"``{name}`` (include/srl_hip.h)."})
        return ""

    def prototype(m):
        ret, name, args = m.groups()
        args = [] if args.strip() == "void" else [ctype(a, name)[0] for a in args.split(",")]
        prototypes[name] = (ctype(ret, name)[0], args)
        return ""

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*define[ \t]+(SRL_\w+)[ \t]+(\S.*?)[ \t]*$", define, text, flags=re.M)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)  # include guards, #include, #ifdef __cplusplus
    text = re.sub(r"\benum\b\s*\w*\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"([\w*][\w\s*]*?)\b(srl_[a-z0-9_]+)\s*\(([^(){};]*)\)\s*;", prototype, text)
    left = re.search(r"\b(srl_[a-z0-9_]+)\s*\(", text)
    if left:
        raise CabiError(f"{left.group(1)}: a declaration the prototype rule cannot read")
    left = re.sub(r'extern\s+"C"\s*\{|\}', "", text).strip()
    if left:
        raise CabiError(f"unparsed text in the header: {left[:80]!r}")
    return consts, structs, prototypes


with open(HEADER) as _f:
    consts, structs, prototypes = parse(_f.read())


def const(name: str) -> int:
    return consts[name]


def struct(name: str):
    return structs[name]
