"""The ctypes signatures of ops/_lib.py against the C entry points they bind.

``_SIGS`` is written by hand; a wrong kind or count there is not an error at load time but silent
argument corruption at the call. This reads every ``RCA_API`` definition out of ``csrc/*.hip``
and checks that ``_SIGS`` names exactly those functions with the same return and argument kinds.
Needs neither the built library nor a GPU.
"""
import ctypes
import glob
import os
import re

from ray_community_amd.ops import _lib

CSRC = os.path.join(os.path.dirname(_lib.__file__), "csrc")
# RCA_API <return type> <name>(<parameters>) {   -- definitions only (a prototype ends in ';')
_DEF = re.compile(r"\bRCA_API\s+([\w\s]+?)\s*\b(rca_\w+)\s*\(([^)]*)\)\s*\{", re.S)
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_longlong, "long long": ctypes.c_longlong,
            "float": ctypes.c_float, "void": None}


def _kind(decl: str, is_param: bool):
    """ctypes kind of one C parameter declaration (with its name) or of a return type."""
    if "*" in decl or "hipStream_t" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if is_param:
        words = words[:-1]  # the parameter's name
    return _SCALARS[" ".join(words)]


def _parse_sources():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            text = re.sub(r"//[^\n]*", "", f.read())
        for ret, name, params in _DEF.findall(text):
            assert name not in found, f"{name} defined twice"
            params = params.strip()
            args = [] if params in ("", "void") else [_kind(p, True) for p in params.split(",")]
            found[name] = (_kind(ret, False), args)
    return found


def test_sigs_match_the_c_definitions():
    c_side = _parse_sources()
    assert sorted(_lib._SIGS) == sorted(c_side)
    for name, (res, args) in _lib._SIGS.items():
        c_res, c_args = c_side[name]
        assert res is c_res, f"{name}: returns {c_res}, _SIGS says {res}"
        assert len(args) == len(c_args), f"{name}: takes {len(c_args)} arguments, _SIGS lists {len(args)}"
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert a is c, f"{name}: argument {i} is {c}, _SIGS says {a}"


def test_parser_kinds():
    assert _kind("const void* q", True) is ctypes.c_void_p
    assert _kind("hipStream_t st", True) is ctypes.c_void_p
    assert _kind("long long sq", True) is ctypes.c_longlong
    assert _kind("long n", True) is ctypes.c_longlong
    assert _kind("float scale", True) is ctypes.c_float
    assert _kind("int B", True) is ctypes.c_int
    assert _kind("void", False) is None
    assert _kind("long long", False) is ctypes.c_longlong
