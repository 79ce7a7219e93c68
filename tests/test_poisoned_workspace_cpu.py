"""RBL_OPT_POISON_WORKSPACE (include/rbl.h), the parts that need no device: the buffer table covers every device buffer of
rbl_ctx, the environment variable sets the option of each new context, and the fill pattern reads as NaN in both precisions."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rigid_body_light_amd", "csrc")
LIB = os.path.join(ROOT, "rigid_body_light_amd", "librbl.so")


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def declared_buffers():
    """RblDevBuf members of struct rbl_ctx (rbl_internal.hpp)"""
    text = _strip_comments(open(os.path.join(CSRC, "rbl_internal.hpp")).read())
    body = re.search(r"struct rbl_ctx\s*\{(.*?)\n\};", text, flags=re.S).group(1)
    names = []
    for decl in re.findall(r"\bRblDevBuf\s+([^;]+);", body):
        names += [n.strip() for n in decl.split(",")]
    return names


def table_rows():
    """(member, kind) rows of kDevBufs (rbl_core.hip)"""
    text = _strip_comments(open(os.path.join(CSRC, "rbl_core.hip")).read())
    table = re.search(r"kDevBufs\[\]\s*=\s*\{(.*?)\n\};", text, flags=re.S).group(1)
    return re.findall(r"\{\s*&rbl_ctx::(\w+)\s*,\s*(RBL_BUF_\w+)\s*\}", table)


def test_every_device_buffer_is_classified_exactly_once():
    names = declared_buffers()
    rows = table_rows()
    assert len(names) >= 40 and len(set(names)) == len(names)
    listed = [m for m, _ in rows]
    for n in names:
        assert listed.count(n) == 1, (n, listed.count(n))
    assert sorted(listed) == sorted(names)
    assert {k for _, k in rows} <= {"RBL_BUF_SCRATCH", "RBL_BUF_PERSIST"}
    kind = dict(rows)
    for n in ("d_gm", "d_part", "d_ens_w"):                    # refilled at every reserve: dead between entry points
        assert kind[n] == "RBL_BUF_SCRATCH", n
    for n in ("d_blkL", "d_blkX", "d_hist", "d_lever", "d_pos", "d_ens", "d_bfPC", "d_ktl", "d_ia", "d_step"):
        assert kind[n] == "RBL_BUF_PERSIST", n                  # carried from one entry point to the next
    # rbl_destroy frees through the same table: no second list of buffers anywhere in the sources
    core = _strip_comments(open(os.path.join(CSRC, "rbl_core.hip")).read())
    assert "RblDevBuf *bufs[]" not in core


_CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.rbl_create.restype = ctypes.c_void_p
lib.rbl_destroy.argtypes = [ctypes.c_void_p]
lib.rbl_option_key.argtypes = [ctypes.c_char_p]
lib.rbl_get_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
k = lib.rbl_option_key(b"poison_workspace")
assert k > 0
h = lib.rbl_create()
v = ctypes.c_int64(-1)
assert lib.rbl_get_option(h, k, ctypes.byref(v)) == 0
lib.rbl_destroy(h)
print(v.value)
"""


def _option_in_fresh_process(env_value):
    env = dict(os.environ)
    env.pop("RBL_POISON_WORKSPACE", None)
    if env_value is not None:
        env["RBL_POISON_WORKSPACE"] = env_value
    out = subprocess.run([sys.executable, "-c", _CHILD, LIB], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return int(out.stdout.strip())


def test_environment_variable_sets_the_option_of_a_new_context():
    assert _option_in_fresh_process("1") == 1
    assert _option_in_fresh_process(None) == 0
    assert _option_in_fresh_process("0") == 0


def test_environment_variable_is_read_at_every_create(monkeypatch):
    lib = ctypes.CDLL(LIB)
    lib.rbl_create.restype = ctypes.c_void_p
    lib.rbl_destroy.argtypes = [ctypes.c_void_p]
    lib.rbl_get_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    k = lib.rbl_option_key(b"poison_workspace")
    got = []
    for val in ("1", None, "1"):
        if val is None:
            monkeypatch.delenv("RBL_POISON_WORKSPACE", raising=False)
        else:
            monkeypatch.setenv("RBL_POISON_WORKSPACE", val)
        h = lib.rbl_create()
        v = ctypes.c_int64(-1)
        assert lib.rbl_get_option(h, k, ctypes.byref(v)) == 0
        got.append(v.value)
        lib.rbl_destroy(h)
    assert got == [1, 0, 1]


def test_pattern_reads_as_nan_in_both_precisions_and_large_as_an_index():
    word = 0x7FF87FF8
    hdr = open(os.path.join(CSRC, "rbl_internal.hpp")).read()
    assert re.search(r"RBL_POISON_WORD\s*=\s*0x7FF87FF8u", hdr)
    raw4 = struct.pack("<I", word)
    assert np.isnan(np.frombuffer(raw4 * 2, dtype=np.float64)[0])
    assert np.isnan(np.frombuffer(raw4, dtype=np.float32)[0])
    assert np.frombuffer(raw4, dtype=np.int32)[0] == 2146992120 > 0
    assert np.frombuffer(raw4, dtype=np.uint32)[0] == 2146992120
