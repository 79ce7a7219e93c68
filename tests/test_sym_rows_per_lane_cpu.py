"""RBL_OPT_SYM_ROWS_PER_LANE admits exactly the row counts a one-vector symmetric kernel is compiled for: 0 (heuristic), 1, 2, 4."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sym_rows_per_lane_values():
    lib = ctypes.CDLL(os.path.join(ROOT, "rigid_body_light_amd", "librbl.so"))
    i64 = ctypes.c_int64
    lib.rbl_create.restype = ctypes.c_void_p
    lib.rbl_destroy.argtypes = [ctypes.c_void_p]
    lib.rbl_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, i64]
    lib.rbl_get_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(i64)]
    lib.rbl_option_key.argtypes = [ctypes.c_char_p]
    h = lib.rbl_create()
    k = lib.rbl_option_key(b"sym_rows_per_lane")
    assert k > 0

    def get():
        v = i64(-1)
        assert lib.rbl_get_option(h, k, ctypes.byref(v)) == 0
        return v.value

    for good in (4, 1, 2, 0):
        assert lib.rbl_set_option(h, k, good) == 0 and get() == good
    for bad in (3, 5, -1):
        assert lib.rbl_set_option(h, k, bad) == 11 and get() == 0      # RBL_ERR_ARG, unchanged
    k2 = lib.rbl_option_key(b"sym2_rows_per_lane")                      # the two-vector kernel has no four-row form
    assert lib.rbl_set_option(h, k2, 4) == 11
    lib.rbl_destroy(h)
