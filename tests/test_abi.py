"""The C-ABI library loads and exports every symbol include/rbl.h declares."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rbl_[a-zA-Z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    names = declared_symbols()
    assert len(names) >= 35
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_context_lifecycle_and_loud_failure_without_device():
    import torch
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    lib.rbl_create.restype = ctypes.c_void_p
    lib.rbl_destroy.argtypes = [ctypes.c_void_p]
    lib.rbl_last_error.restype = ctypes.c_char_p
    lib.rbl_last_error.argtypes = [ctypes.c_void_p]
    lib.rbl_precision.restype = ctypes.c_char_p
    assert lib.rbl_precision() == b"double"
    h = lib.rbl_create()
    assert h
    lib.rbl_apply_M.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p]
    buf = (ctypes.c_double * 6)(*([0.0] * 6))
    rc = lib.rbl_apply_M(h, buf, buf, 6, buf)
    assert rc == 7 and b"setParameters" in lib.rbl_last_error(h)     # RBL_ERR_STATE
    if torch.cuda.device_count() == 0:
        lib.rbl_set_parameters.argtypes = [ctypes.c_void_p] + [ctypes.c_double] * 4 + [ctypes.c_void_p, ctypes.c_int]
        cfg = (ctypes.c_double * 6)(0, 0, 1, 0, 0, -1)
        assert lib.rbl_set_parameters(h, 1.0, 0.1, 1.0, 1.0, cfg, 2) == 0
        rc = lib.rbl_apply_M(h, buf, buf, 6, buf)
        assert rc == 5 and b"no CPU fallback" in lib.rbl_last_error(h)  # RBL_ERR_NO_DEVICE
    lib.rbl_destroy(h)


def option_keys():
    """RBL_OPT_* enumerators of include/rbl.h -> {name: value}"""
    text = open(os.path.join(ROOT, "include", "rbl.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(RBL_OPT_[A-Z0-9_]+)\s*=\s*(\d+)", text)}


def test_every_option_is_named_bounded_and_round_trips(monkeypatch):
    """include/rbl.h's named options (the replacement of the rounds 1-3 switchboard of magic integers): every key 1 .. RBL_OPT_COUNT - 1 has a
    table row (name, range, default), starts at its default, round-trips its extreme values, rejects values outside its range
    and unknown keys with RBL_ERR_ARG leaving the option unchanged; a value inside the range that selects nothing (sym_waves = 2, 3)
    is rejected the same way; the switchboard of magic integers of rounds 1-3 is gone from the library."""
    i64 = ctypes.c_int64
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    lib.rbl_create.restype = ctypes.c_void_p
    lib.rbl_destroy.argtypes = [ctypes.c_void_p]
    lib.rbl_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, i64]
    lib.rbl_get_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(i64)]
    lib.rbl_option_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)] + [ctypes.POINTER(i64)] * 3
    lib.rbl_option_key.argtypes = [ctypes.c_char_p]
    monkeypatch.delenv("RBL_POISON_WORKSPACE", raising=False)      # (it sets poison_workspace's starting value)
    keys = option_keys()
    count = keys.pop("RBL_OPT_COUNT")
    assert sorted(keys.values()) == list(range(1, count)), "RBL_OPT_* keys must be 1 .. RBL_OPT_COUNT - 1 without gaps"
    h = lib.rbl_create()

    def get(k):
        v = i64(-12345)
        assert lib.rbl_get_option(h, k, ctypes.byref(v)) == 0
        return v.value

    names = set()
    for enum_name, k in sorted(keys.items(), key=lambda kv: kv[1]):
        nm, lo, hi, df = ctypes.c_char_p(), i64(), i64(), i64()
        assert lib.rbl_option_info(k, ctypes.byref(nm), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(df)) == 0, enum_name
        name = nm.value.decode()
        assert name and name not in names and "RBL_OPT_" + name.upper() == enum_name
        names.add(name)
        assert lib.rbl_option_key(name.encode()) == k
        assert lo.value <= df.value <= hi.value
        assert get(k) == df.value, name                                  # a fresh context holds the defaults
        for v in (lo.value, hi.value, df.value):
            assert lib.rbl_set_option(h, k, v) == 0 and get(k) == v, (name, v)
        for bad in (lo.value - 1, hi.value + 1):
            assert lib.rbl_set_option(h, k, bad) == 11 and get(k) == df.value, (name, bad)   # RBL_ERR_ARG, unchanged
    for bad_key in (0, count, -3, 1000):
        v = i64(7)
        assert lib.rbl_set_option(h, bad_key, 1) == 11
        assert lib.rbl_get_option(h, bad_key, ctypes.byref(v)) == 11 and v.value == 7
        assert lib.rbl_option_info(bad_key, None, None, None, None) == 11
    assert lib.rbl_option_key(b"no_such_option") == 0
    kw = lib.rbl_option_key(b"sym_waves")
    for bad in (2, 3):                                                    # inside [0, 4] but no kernel has that many waves
        assert lib.rbl_set_option(h, kw, bad) == 11 and get(kw) == 0
    for good in (1, 4, 0):
        assert lib.rbl_set_option(h, kw, good) == 0 and get(kw) == good
    assert not hasattr(lib, "rbl_set_" + "tuning")
    lib.rbl_destroy(h)


def test_communicator_entry_points_without_a_device():
    """rbl_comm_*: argument checks and the no-communicator state work without a GPU; the collectives themselves are GPU tests."""
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    lib.rbl_create.restype = ctypes.c_void_p
    lib.rbl_destroy.argtypes = [ctypes.c_void_p]
    lib.rbl_comm_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
    lib.rbl_comm_init_rccl.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.rbl_set_comm_ops.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.rbl_comm_finalize.argtypes = [ctypes.c_void_p]
    h = lib.rbl_create()
    r, w, k = ctypes.c_int(9), ctypes.c_int(9), ctypes.c_int(9)
    assert lib.rbl_comm_info(h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(k)) == 0 and (r.value, w.value, k.value) == (0, 1, 0)
    ident = (ctypes.c_char * 128)()
    assert lib.rbl_comm_init_rccl(h, ident, 2, 2) == 11          # rank out of range
    assert lib.rbl_comm_init_rccl(h, None, 0, 1) == 11
    assert lib.rbl_set_comm_ops(h, 3, 2, None, None, None) == 11
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    cb = CB(lambda user, buf, n: 0)
    assert lib.rbl_set_comm_ops(h, 1, 2, ctypes.cast(cb, ctypes.c_void_p), None, None) == 0
    assert lib.rbl_comm_info(h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(k)) == 0 and (r.value, w.value, k.value) == (1, 2, 1)
    assert lib.rbl_comm_finalize(h) == 0
    assert lib.rbl_comm_info(h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(k)) == 0 and (r.value, w.value, k.value) == (0, 1, 0)
    lib.rbl_destroy(h)


def test_isa_counts_match_the_kernel_sources():
    """bench.py prices its roofline with per-pair instruction counts taken from the assembly of the SAME kernel sources the
    library is built from (tools/isa_stats.py, run by rigid_body_light_amd/build.py): the file exists, belongs to the
    current sources (hash) and holds the kernels the default benchmark launches."""
    import hashlib
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = json.load(open(os.path.join(root, "rigid_body_light_amd", "librbl.isa.json")))
    h = hashlib.sha256()
    for f in ("rbl_kernels.hip", "rbl_pair.hpp"):
        h.update(open(os.path.join(root, "rigid_body_light_amd", "csrc", f), "rb").read())
    assert d["kernel_source_sha256"] == h.hexdigest(), "run rigid_body_light_amd/build.py"
    for k in ("k_apply_M_sym<true,2>", "k_apply_M_sym<false,2>", "k_apply_M_sym<true,1>", "k_apply_M_sym2<true,2>"):
        p = d["kernels"][k]["per_unordered_pair"]
        assert 30 < p["valu"] < 130 and p["flop"] <= 2 * p["valu"] and p["fma"] > p["mul"]
    sys.path.insert(0, root)
    import bench
    assert bench.isa_counts("k_apply_M_sym<true,2>")["flop"] == d["kernels"]["k_apply_M_sym<true,2>"]["per_unordered_pair"]["flop"]
    # the HBM-traffic figure of the bench line comes from PMC passes under profiles/, taken from the kernel code a build
    # held then (instruction-text hash of the profiled instance).  After a kernel change bench.py must stop quoting it
    # (traffic: null) until the passes are re-taken (profiles/README.md) -- a stale profile is a warning here, not a failure:
    # correctness tests do not depend on a perf artefact
    import glob
    import warnings
    files = sorted(glob.glob(os.path.join(root, "profiles", "r0*_bench_cfg3_pmc.json")))
    pmc = json.load(open(files[-1]))
    got = bench.pmc_traffic("k_apply_M_sym<true,2>", "cfg3", 1)[0]
    if pmc["kernel_isa_sha256"] == d["instance_isa_sha256"].get(pmc["kernel_instance"]):
        assert got == pmc["hbm_bytes_per_launch"]
    else:
        warnings.warn("profiles/%s was taken from other kernel code than this build holds: re-run the PMC passes" % os.path.basename(files[-1]))
        assert got is None or got != pmc["hbm_bytes_per_launch"]
