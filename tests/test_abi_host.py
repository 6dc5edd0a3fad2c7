"""CPU tests (no GPU) of the C ABI: every header under include/ against its entry of ``_lib.ABIS``, one case per header.

This file replaces the per-header pairs ``test_*_header_compiles_as_c_and_struct_sizes_match_the_binding`` and
``test_*_exports_every_declared_symbol*`` that tests/test_host_logic.py and the ten ``test_*_host.py`` files of the sub-headers carried.  What they
asserted, and where it is asserted now:

 * the header compiles alone as C99 with -Wall -Werror            -> test_header_compiles_and_every_struct_matches_its_mirror (the same gcc call)
 * the header's typedef'd struct names equal a hand-written dict   -> same test, against ``abi.structs``
 * sizeof of every struct equals the mirror's                      -> same test
 * offsetof of two to four chosen fields (all of them in two files) -> same test, for EVERY field of every struct, with the field's size, after
                                                                       the ordered field names of header and mirror were compared
 * the header's version #define equals ``_lib.AID_*_ABI_VERSION``  -> test_exports_version_and_macros, against ``abi.version`` and the literal VERSIONS
 * AID_RESTORE_JOB_FIELDS / AID_SPEC_ITEM_FIELDS equal their #define -> same test, for every name of ``abi.macros``
 * the declared functions equal ``_lib.*_EXPORTS`` (and a literal set in six files) -> same test, against ``abi.exports`` and the literal PINNED
 * they share no name with the lists that existed at the time      -> test_no_symbol_and_no_struct_appears_under_two_headers, over the whole table
 * the built library exports every declared symbol                 -> test_exports_version_and_macros
 * ``lib().aid_*_abi_version()`` equals the binding's (and the literal 14 / 1 of a few neighbours) -> same test (VERSIONS pins all eleven)
 * ``pack_dims`` values at the end of test_c_abi_exports_every_declared_symbol -> tests/test_host_logic.py::test_pack_dims_of_the_library
New here: the prototypes (a launch entry names the struct the table gives it; a host query has the restype and argtypes the table gives it) and that
every header under include/ has an entry."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
# Pinned here on purpose: a version changed in a header and in the binding together still shows up as an edit to this test
VERSIONS = {"aid_kernels.h": 14, "aid_degrade.h": 1, "aid_phase.h": 1, "aid_autoregressive.h": 1, "aid_restore.h": 1, "aid_declip.h": 1,
            "aid_resample_op.h": 1, "aid_bwe_long.h": 1, "aid_lowrate_long.h": 1, "aid_phase_long.h": 1, "aid_spec_long.h": 1}
# Entry points a header must keep declaring, whatever header and table say together (the literal sets of the tests this file replaces)
PINNED = {"aid_autoregressive.h": {"aid_ar_carry"}, "aid_restore.h": {"aid_window_gather", "aid_window_scatter"},
          "aid_declip.h": {"aid_declip_abi_version", "aid_clip_known", "aid_declip_gather"}, "aid_resample_op.h": {"aid_resample_poly_adj"},
          "aid_bwe_long.h": {"aid_bwe_long_abi_version", "aid_fir_observed", "aid_bwe_gather"},
          "aid_lowrate_long.h": {"aid_lowrate_long_abi_version", "aid_rate_observed", "aid_lowrate_gather"},
          "aid_phase_long.h": {"aid_phase_long_abi_version", "aid_stft_mag_observed", "aid_pr_gather"},
          "aid_spec_long.h": {"aid_spec_long_abi_version", "aid_stft_mask_observed", "aid_spec_gather"}}
# The one field a mirror may name differently: ``in`` is a Python keyword
RENAMED = {("aid_fft_pass_params", "in"): "inp"}
C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "void": None, "const char*": ctypes.c_char_p, "int*": ctypes.POINTER(ctypes.c_int)}


def _abis():
    from audio_inpainting_diffusion_amd import _lib
    return _lib.ABIS


def _abi(header):
    return next(a for a in _abis() if a.header == header)


def _code(header):
    """the header's text without its comments"""
    text = open(os.path.join(INCLUDE, header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _c_structs(code):
    """{typedef name: [field names in order]} of every ``typedef struct { ... } aid_*;``"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(aid_\w+)\s*;", code, flags=re.S):
        decls = [d for d in (d.strip() for d in body.split(";")) if d]
        out[name] = [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", part).group(1) for d in decls for part in d.split(",")]
    return out


def _c_functions(code):
    """{name: (return type, [argument types])} of every function the header declares"""
    out = {}
    for ret, name, args in re.findall(r"^\s*(int|int64_t|void|const char\*)\s+(aid_\w+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        args = [] if args.strip() == "void" else [re.sub(r"\s*\w+\s*$", "", a.strip()) for a in args.split(",")]
        out[name] = (ret, args)
    return out


def test_every_header_has_one_entry_and_every_size_and_offset_is_compared():
    abis = _abis()
    assert sorted(a.header for a in abis) == sorted(os.listdir(INCLUDE)) == sorted(VERSIONS) and abis[0].header == "aid_kernels.h"
    structs = [cls for a in abis for cls in a.structs.values()]
    n = sum(1 + len(cls._fields_) for cls in structs)
    print(f"{len(abis)} headers, {len(structs)} structs: {n} sizeof / offsetof comparisons against gcc (plus one size per field)")
    assert len(structs) == 56 and n >= 758


def test_no_symbol_and_no_struct_appears_under_two_headers():
    for what in ("exports", "structs"):
        names = [n for a in _abis() for n in getattr(a, what)]
        assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)


@pytest.mark.parametrize("header", sorted(VERSIONS))
def test_header_compiles_and_every_struct_matches_its_mirror(header, tmp_path):
    """The header must compile as plain C99 on its own, declare exactly the structs of its table entry, and every struct must have the ordered field
    names, the size, and at every field the offset and field size of its ctypes mirror (a reordered pair of same-sized fields passes a sizeof check)."""
    abi = _abi(header)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    c_structs = _c_structs(_code(header))
    assert set(c_structs) == set(abi.structs), set(c_structs) ^ set(abi.structs)
    for c, cls in abi.structs.items():
        assert [RENAMED.get((c, f), f) for f in c_structs[c]] == [f for f, _ in cls._fields_], c
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void) {{\n' +
                   "".join(f'    printf("{c} %zu\\n", sizeof({c}));\n' for c in c_structs) +
                   "".join(f'    printf("{c}.{f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c}*)0)->{f}));\n' for c, fs in c_structs.items() for f in fs) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-o", str(exe)])
    out = {k: tuple(int(v) for v in vs) for k, *vs in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    for c, cls in abi.structs.items():
        assert out[c] == (ctypes.sizeof(cls),), (c, out[c], ctypes.sizeof(cls))
        for f in c_structs[c]:
            field = getattr(cls, RENAMED.get((c, f), f))
            assert out[f"{c}.{f}"] == (field.offset, field.size), (c, f, out[f"{c}.{f}"], field.offset, field.size)


@pytest.mark.parametrize("header", sorted(VERSIONS))
def test_exports_version_and_macros(header):
    """header <=> table <=> library: the functions the header declares are the table's, with the prototypes the table gives them; the built library
    exports them; the version #define, the version function and the table agree with the version pinned above; every mirrored macro has its value."""
    from audio_inpainting_diffusion_amd import _lib
    abi, code = _abi(header), _code(header)
    funcs = _c_functions(code)
    assert set(funcs) == set(abi.exports), set(funcs) ^ set(abi.exports)
    assert PINNED.get(header, set()) <= set(funcs) and (header != "aid_kernels.h" or len(funcs) >= 15)
    c_name = {cls: c for c, cls in abi.structs.items()}
    for name, cls in abi.launches.items():
        assert funcs[name] == ("int", [f"const {c_name[cls]}*", "void*"]), (name, funcs[name])
    for name, (restype, argtypes) in {abi.version_fn: (ctypes.c_int, []), **abi.queries}.items():
        assert (C_TYPES[funcs[name][0]], [C_TYPES[a] for a in funcs[name][1]]) == (restype, argtypes), (name, funcs[name])
    so = os.path.join(ROOT, "audio_inpainting_diffusion_amd", "libaid_hip.so")
    if not os.path.exists(so):
        import build
        build.build()
    lib = ctypes.CDLL(so)
    for name in funcs:
        assert hasattr(lib, name), f"{name} declared in {header} but not exported"
    define = int(re.search(r"#define %s (\d+)" % abi.version_fn.upper(), code).group(1))
    assert define == getattr(_lib.lib(), abi.version_fn)() == abi.version == VERSIONS[header]
    for macro in abi.macros:
        assert int(re.search(r"#define %s (\d+)" % macro, code).group(1)) == getattr(_lib, macro), macro
