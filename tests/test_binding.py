"""coponerf_amd/_hip.py derives the whole ctypes binding from include/coponerf_hip.h: the parser on a header written here, the
real header's prototypes by type form, and the argument count of every kernel call site in the package and the tests."""
import ast
import collections
import ctypes
import glob
import os

import pytest

from coponerf_amd import _hip

I, F, D, LL, P = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p
PP = ctypes.POINTER(ctypes.c_void_p)

HEADER = """
/* a header in the forms include/coponerf_hip.h uses
 * int cpn_in_a_comment(int a);   <- not a declaration */
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define CPN_PLAIN 12   /* a trailing comment (with parentheses) */
#define CPN_NEG   (-2)
#define CPN_EXPR (128 * 32 + 3 * (16 - 4))
#define CPN_NAME_ONLY
#define CPN_NOT_INT 1.5f
#define CPN_FROM_OTHER (CPN_PLAIN + 1)
#define OTHER_PREFIX 7
int         cpn_version(void);
int cpn_empty();
const char* cpn_message(void);
long long cpn_count(int n, long long rows);
int cpn_scalars(int a, float b, double c, long long d, const int e);
int cpn_pointers(const float* x, uint8_t *y, const float* const* host_list, void* stream, const void* segs);
int cpn_stream_out(int first, void** stream_out);
int cpn_broken(const float* x,   /* a comment between the lines */
               long long n,
               float* y, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_form():
    protos, consts = _hip.parse_header(HEADER)
    assert protos == {
        "cpn_version": (I, []),
        "cpn_empty": (I, []),
        "cpn_message": (ctypes.c_char_p, []),
        "cpn_count": (LL, [I, LL]),
        "cpn_scalars": (I, [I, F, D, LL, I]),
        "cpn_pointers": (I, [P, P, P, P, P]),
        "cpn_stream_out": (I, [I, PP]),
        "cpn_broken": (I, [P, LL, P, P]),
    }
    assert list(protos) == ["cpn_version", "cpn_empty", "cpn_message", "cpn_count", "cpn_scalars", "cpn_pointers", "cpn_stream_out",
                            "cpn_broken"]
    assert consts == {"PLAIN": 12, "NEG": -2, "EXPR": 128 * 32 + 3 * (16 - 4)}
    assert all(type(v) is int for v in consts.values())


@pytest.mark.parametrize("line", [
    "int cpn_x(int a, unsigned b);",                      # a scalar type the table does not have
    "int cpn_x(int a, size_t);",
    "void cpn_x(int a);",
    "int* cpn_x(int a);",
    "int cpn_x(int a, float b)",                          # cpn_x( that is no complete prototype: no semicolon
    "int cpn_x(int a, float b) { return 0; }",
    "int cpn_x(int a, void (*done)(int), void* stream);",  # a function-pointer parameter
    "int cpn_x(int a, float v[3]);",
    "int cpn_x(int a, ...);",
    "int cpn_version(int again);",                        # declared twice
])
def test_parser_raises_on_what_it_cannot_read(line):
    assert "int cpn_empty();" in HEADER
    with pytest.raises(_hip.HeaderError):
        _hip.parse_header(HEADER.replace("int cpn_empty();", line))


def test_real_header_by_type_form():
    pr = _hip.PROTOTYPES
    assert len(pr) >= 109 and _hip.declared_symbols() == sorted(pr)
    assert all(_hip.SIGNATURES[n] == a for n, (_, a) in pr.items()) and set(_hip.SIGNATURES) == set(pr)
    ret, args = pr["cpn_adam_step"]
    assert ret is I and len(args) == 14 and args[9:13] == [D] * 4 and args[:2] == [P, P] and args[2] is I and args[13] is P
    assert pr["cpn_project_rays"] == (I, [P, P, LL, I, I, I, P, P, P, P])
    assert pr["cpn_gn_stats_doubles"] == (LL, [I, I, LL])
    assert pr["cpn_last_error"] == (ctypes.c_char_p, [])
    assert pr["cpn_abi_version"] == (I, [])
    assert pr["cpn_stream_create_cu_range"] == (I, [I, I, PP])
    assert pr["cpn_lpips_head"] == (I, [P] * 5 + [I, I] + [P] * 4)
    assert pr["cpn_pose_positional"][1][3] is F and pr["cpn_select_rays"][1][2] is F
    assert pr["cpn_pose_tail"][1][3] is P                                   # const float* const*: a host array, not void**


def test_constants_come_from_the_header():
    c = _hip.CONSTANTS
    for name, value in c.items():
        assert getattr(_hip, name) == value and type(value) is int, name
    assert (_hip.ABI_VERSION, _hip.CAM_STRIDE, _hip.TAB_LD, _hip.RAYC_STRIDE, _hip.ADAM_SEG_BYTES) == (12, 96, 832, 64, 48)
    assert (_hip.CAM_TQ, _hip.CAM_M, _hip.CAM_AOWN, _hip.CAM_AOTH, _hip.CAM_KQ, _hip.CAM_KC, _hip.CAM_KO, _hip.CAM_KN) == \
        (0, 16, 32, 48, 64, 68, 72, 76)
    assert _hip.LIGHTFIELD_PACK_FLOATS == 128 * 32 + 128 + 3 * (128 * 416 + 128 + 2 * (128 * 128 + 128)) + 16 * 128 + 16
    assert _hip.ENC_FRAG_HALVES == 13 * 3 * 4 * 64 * 8 and _hip.LPIPS_LAYERS == 5 and _hip.POSE_TAIL_TENSORS == 16
    assert (c["E_ARG"], c["E_SHAPE"]) == (-1, -2)
    from coponerf_amd import lpips
    assert lpips.LAYERS == _hip.LPIPS_LAYERS


# ---- call sites ---------------------------------------------------------------------------------------------------------
# ctypes lets surplus arguments of a cdecl call through, so a call site left behind by a signature that shrank would only show on
# the GPU.  Every call("cpn_...", ...) / _hip.call("cpn_...", ...) with a literal name and every direct <lib>.cpn_...(...) call in
# the package and the tests passes as many arguments as the header declares.  A site that spreads a tuple cannot be counted:
# these are all of them, (file, function, entry point) -> sites, and a new one fails until it is listed here.
STARRED = {
    ("coponerf_amd/render.py", "run_chunk", "cpn_attend_units"): 2,
    ("coponerf_amd/render.py", "run_chunk", "cpn_local_units"): 2,
    ("coponerf_amd/train_f32.py", "backward", "cpn_gemm_f16_combine_hs"): 1,
    ("coponerf_amd/train_f32.py", "backward", "cpn_hid_grad_combine"): 1,
    ("coponerf_amd/train_fns.py", "backward", "cpn_gemm_f16_combine"): 1,
    ("coponerf_amd/train_fns.py", "backward", "cpn_hid_grad_combine"): 1,
    ("tests/test_gpu_attend_units.py", "_run_both", "cpn_attend_units"): 1,
    ("tests/test_gpu_attend_units.py", "_run_both", "cpn_local_units"): 1,
    ("tests/test_gpu_attend_units.py", "with_the_pair", "cpn_attend_hidden"): 1,
    ("tests/test_gpu_attend_units.py", "with_the_pair", "cpn_local_units"): 1,
    ("tests/test_gpu_auto.py", "enc", "cpn_encode_hidden_f32"): 1,
    ("tests/test_gpu_auto.py", "enc", "cpn_encode_hidden_f32_rays"): 1,
    ("tests/test_gpu_logits_f64.py", "_attend_units", "cpn_attend_units"): 1,
    ("tests/test_gpu_logits_f64.py", "_local_units", "cpn_local_units"): 1,
    ("tests/test_gpu_logits_f64.py", "run", "cpn_sample_geometry"): 1,
    ("tests/test_gpu_logits_f64.py", "test_attend_units_at_the_lds_limit", "cpn_attend_units"): 1,
    ("tests/test_gpu_parity.py", "_encode_first_layer", "cpn_encode_key"): 1,
    ("tests/test_gpu_parity.py", "test_encode_key_entry_is_bit_identical", "cpn_encode_key"): 2,
    ("tests/test_ssim_ref.py", "test_new_symbols_are_declared_and_exported", "cpn_ssim_warp"): 3,
    ("tests/test_ssim_ref.py", "test_new_symbols_are_declared_and_exported", "cpn_ssim_warp_bwd"): 2,
}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call_sites(path):
    """(function, entry point, number of arguments or None when one is starred, line) of every kernel call in a file"""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    sites = []

    def walk(node, func):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            func = node.name
        if isinstance(node, ast.Call):
            f, args, name = node.func, node.args, None
            if isinstance(f, ast.Attribute) and f.attr.startswith("cpn_"):
                name = f.attr
            elif (f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None) == "call" and args and \
                    isinstance(args[0], ast.Constant) and isinstance(args[0].value, str) and args[0].value.startswith("cpn_"):
                name, args = args[0].value, args[1:]
            if name is not None:
                assert not node.keywords, f"{path}:{node.lineno}: keyword arguments in a kernel call"
                sites.append((func, name, None if any(isinstance(a, ast.Starred) for a in args) else len(args), node.lineno))
        for child in ast.iter_child_nodes(node):
            walk(child, func)

    walk(tree, "<module>")
    return sites


def test_call_site_walk_sees_each_form(tmp_path):
    src = tmp_path / "m.py"
    src.write_text('def f(r):\n    call("cpn_a", 1, 2)\n    _hip.call("cpn_b", 0, *r)\n    x = _hip.lib().cpn_c(1)\n'
                   '    _call("cpn_d", 1)\n    call(name, 1)\nlib.cpn_e()\n')
    assert [s[:3] for s in _call_sites(str(src))] == [("f", "cpn_a", 2), ("f", "cpn_b", None), ("f", "cpn_c", 1),
                                                      ("<module>", "cpn_e", 0)]


def test_call_sites_pass_the_declared_number_of_arguments():
    files = sorted(glob.glob(os.path.join(ROOT, "coponerf_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")))
    counted, starred, wrong = 0, collections.Counter(), []
    for path in files:
        rel = os.path.relpath(path, ROOT).replace(os.sep, "/")
        for func, name, nargs, line in _call_sites(path):
            if name not in _hip.PROTOTYPES:
                wrong.append(f"{rel}:{line}: {name} is not declared in the header")
            elif nargs is None:
                starred[(rel, func, name)] += 1
            else:
                counted += 1
                if nargs != len(_hip.PROTOTYPES[name][1]):
                    wrong.append(f"{rel}:{line}: {name} takes {len(_hip.PROTOTYPES[name][1])} arguments, {nargs} passed")
    assert not wrong, "\n".join(wrong)
    assert counted >= 134                                                 # the walk finds the calls (134 in the package alone)
    assert dict(starred) == STARRED, sorted(set(starred.items()) ^ set(STARRED.items()))
    assert sum(n for (rel, _, _), n in STARRED.items() if rel.startswith("coponerf_amd/")) == 8
