"""srl_amd/cabi.py against a real C compiler: the ctypes Structures, field by field, and every constant it read from
include/srl_hip.h are compared with what a host program compiled against that header prints; and the parser refuses what it
cannot read.  Host-only: the probe includes the header and loads no library."""
import ctypes
import os
import shutil
import subprocess

import pytest

from srl_amd import cabi

C_NAMES = {py: c for c, py in cabi.RENAMES.items()}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """{"sizeof": {struct: n}, "field": {(struct, field): (offset, size)}, "const": {name: value}} as the compiler sees them."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "srl_hip.h"', "int main(void) {"]
    for name, cls in cabi.structs.items():
        lines.append(f'  printf("sizeof {name} - %zu 0\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            c = C_NAMES.get(field, field)
            lines.append(f'  printf("field {name} {field} %zu %zu\\n", offsetof({name}, {c}), sizeof((({name}*)0)->{c}));')
    for name in cabi.consts:
        lines.append(f'  printf("const {name} - %lld 0\\n", (long long){name});')
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("cabi_probe")
    src, exe = d / "probe.c", d / "probe"
    src.write_text("\n".join(lines) + "\n")
    cc = next((c for c in (["cc"], ["gcc"], ["hipcc", "-x", "c"]) if shutil.which(c[0])), None)
    assert cc is not None, "no host C compiler (cc, gcc, hipcc) to check the struct layouts with"
    subprocess.run(cc + ["-std=c99", "-I", os.path.dirname(cabi.HEADER), "-o", str(exe), str(src)], check=True)
    out = {"sizeof": {}, "field": {}, "const": {}}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, owner, field, a, b = ln.split()
        out[kind][(owner, field) if kind == "field" else owner] = (int(a), int(b)) if kind == "field" else int(a)
    return out


def test_struct_layouts_match_the_compiler(probe):
    assert len(cabi.structs) >= 9 and probe["sizeof"].keys() == cabi.structs.keys()
    for name, cls in cabi.structs.items():
        assert ctypes.sizeof(cls) == probe["sizeof"][name], name
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            assert (d.offset, d.size) == probe["field"][(name, field)], (name, field)
    assert len(probe["field"]) == sum(len(c._fields_) for c in cabi.structs.values())
    # the two sizes the binding has always pinned, and the renames Python forces
    assert probe["sizeof"]["srl_ppo_hparams"] == 44 and probe["sizeof"]["srl_gemm_desc"] == 208
    assert cabi.RENAMES == {"in": "in_"} and hasattr(cabi.struct("srl_mlp_layer"), "in_")


def test_constants_match_the_compiler(probe):
    assert probe["const"] == cabi.consts
    assert cabi.const("SRL_EATTN_KEY_B") == 13 and cabi.const("SRL_LT_COUNT") == 10 and cabi.const("SRL_FAMILY_CHANNELS_LAST") == 4


def test_header_counts_and_type_map():
    assert len(cabi.prototypes) >= 139 and len(cabi.structs) >= 9
    vp, P = ctypes.c_void_p, ctypes.POINTER
    assert cabi.prototypes["srl_abi_version"] == (ctypes.c_int, [])
    assert cabi.prototypes["srl_last_error"] == (ctypes.c_char_p, [])
    assert cabi.prototypes["srl_device_info"] == (ctypes.c_int, [vp, vp, ctypes.c_char_p, ctypes.c_int])
    assert cabi.prototypes["srl_gae_scan_workspace_bytes"] == (ctypes.c_long, [ctypes.c_int, ctypes.c_int])
    assert cabi.prototypes["srl_gae_scan_plan"] == (ctypes.c_int, [ctypes.c_int] * 6 + [vp])      # int32_t* out
    assert cabi.prototypes["srl_gemm"] == (ctypes.c_int, [vp, P(cabi.struct("srl_gemm_desc"))])
    assert cabi.prototypes["srl_step_plan_create"] == (ctypes.c_int, [vp, vp])                       # void**
    assert cabi.prototypes["srl_accumulate_n"][1] == [vp, vp, vp, ctypes.c_int32, ctypes.c_int64]    # const float* const*
    assert cabi.prototypes["srl_polyak_update"][1] == [vp, vp, vp, ctypes.c_int64, ctypes.c_double]
    assert cabi.prototypes["srl_instr_lstm_bwd_workspace"] == (ctypes.c_int64, [P(cabi.struct("srl_instr_lstm")), ctypes.c_int64])


def test_parser_reads_the_headers_grammar():
    consts, structs, protos = cabi.parse("""
        #define SRL_N 3   /* a comment */
        enum { SRL_A, SRL_B, SRL_C = 7, SRL_D };
        enum srl_kind { SRL_K0 = 2, SRL_K1 };
        typedef struct srl_t {
          int32_t in, out; const float* w[SRL_N];
          int64_t ld_a, ld_b[SRL_K1], ld_c;
          float *ga, *gb; uint8_t flag; double x[2];
        } srl_t;
        int64_t srl_f(const srl_t* d, const float* const* srcs, void** out, const char* name, long n);
        int srl_g(void);
    """)
    assert consts == dict(SRL_N=3, SRL_A=0, SRL_B=1, SRL_C=7, SRL_D=8, SRL_K0=2, SRL_K1=3)      # an enum without `=` counts up
    t = structs["srl_t"]
    assert [f for f, _ in t._fields_] == ["in_", "out", "w", "ld_a", "ld_b", "ld_c", "ga", "gb", "flag", "x"]  # two declarators, two fields
    assert t.w.size == 3 * ctypes.sizeof(ctypes.c_void_p) and t.ld_b.size == 24 and t.ld_c.offset == t.ld_b.offset + 24  # extents by constant
    assert t.gb.size == ctypes.sizeof(ctypes.c_void_p) and t.out.offset == 4 and t.x.size == 16
    assert protos["srl_f"] == (ctypes.c_int64, [ctypes.POINTER(t), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_long])
    assert protos["srl_g"] == (ctypes.c_int, [])


@pytest.mark.parametrize("snippet, named", [
    ("int srl_f(size_t n);", "size_t"),                                          # an unknown scalar type
    ("int srl_f(const srl_missing* d);", "srl_missing"),                         # a pointer to a struct that was not parsed
    ("typedef struct srl_t { unsigned x; } srl_t;", "unsigned"),                 # an unknown field type
    ("int srl_foo(int (*cb)(int));", "srl_foo"),                                 # a prototype outside the grammar
    ("int srl_foo(int a)\n{ return a; }", "srl_foo"),                            # not a declaration
    ("typedef struct srl_t { int32_t a[SRL_NOPE]; } srl_t;", "SRL_NOPE"),        # an extent that does not resolve
    ("#define SRL_X (1 << 3)", "SRL_X"),                                         # a non-literal #define
    ("enum { SRL_A = 1 << 2 };", "SRL_A"),
    ("typedef struct srl_t { int32_t a; } srl_u;", "srl_u"),
    ("int srl_f(void); struct srl_s { int a; };", "struct"),                     # anything left over
])
def test_parser_refuses_what_it_cannot_read(snippet, named):
    with pytest.raises(cabi.CabiError, match=named):
        cabi.parse(snippet)
