"""The packed scorer's cell-form rule and the self-test of its flag form: libswmi_pk_form.so (include/swmi_pk_form.h, DESIGN.md
section 5a).  Reached as swmi.pk_form.<name>.  cell_form needs no device and no swmi.init; selftest_max3_negative runs on the
current HIP device."""
import ctypes
import os

import numpy as np

from . import ERR_DOMAIN, SwmiError

FORM_Q0, FORM_BIAS, FORM_VERT, FORM_FLAG = 0, 1, 2, 3
FORM_NAMES = ("q0", "bias", "vert", "flag")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWMI_PK_FORM_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libswmi_pk_form.so"))

_lib = None


def load():
    """dlopen libswmi_pk_form.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError("%s not found: run make -C smith-waterman-simd_amd/csrc" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.swmi_pk_cell_form.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.swmi_pk_selftest_max3_negative.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
    lib.swmi_pk_product_form.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.swmi_pk_selftest_product_mad.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
    _lib = lib
    return lib


def cell_form(score_matrix, gap_penalty):
    """swmi_pk_cell_form: (form, m + gap, rescaled gap) -- form one of FORM_Q0, FORM_BIAS, FORM_VERT, FORM_FLAG (the flag form of
    the vertical-offset kernel: its name, the q0 cell); the two scale figures are 0 unless the form is FORM_FLAG."""
    sm = np.ascontiguousarray(np.asarray(score_matrix).reshape(16))
    if sm.min() < -128 or sm.max() > 127:
        raise SwmiError(ERR_DOMAIN, "score_matrix entries must fit int8")
    sm = sm.astype(np.int8)
    scale = (ctypes.c_int * 2)()
    rc = load().swmi_pk_cell_form(sm.ctypes.data, int(gap_penalty), scale)
    if rc < 0:
        raise SwmiError(rc, "swmi_pk_cell_form: gap_penalty %d outside [0, 127]" % int(gap_penalty))
    return rc, scale[0], scale[1]


def product_form(score_matrix, gap_penalty):
    """swmi_pk_product_form: (eligible, row multipliers a[4], column multipliers b[4], verified bound) -- eligible is True when the
    set's flag form runs as the product form (one 16-bit multiply-add per row for lookup and diagonal add); the constants are
    zeros when it is not."""
    sm = np.ascontiguousarray(np.asarray(score_matrix).reshape(16))
    if sm.min() < -128 or sm.max() > 127:
        raise SwmiError(ERR_DOMAIN, "score_matrix entries must fit int8")
    sm = sm.astype(np.int8)
    consts = (ctypes.c_int * 9)()
    rc = load().swmi_pk_product_form(sm.ctypes.data, int(gap_penalty), consts)
    if rc < 0:
        raise SwmiError(rc, "swmi_pk_product_form: gap_penalty %d outside [0, 127]" % int(gap_penalty))
    return bool(rc), tuple(consts[0:4]), tuple(consts[4:8]), consts[8]


def selftest_product_mad():
    """(comparisons made, mismatches) of swmi_pk_selftest_product_mad: v_pk_mad_i16 with the product form's constants, every
    (row base, column base), every H up to the verified bound, both halves, and the max3 behind it."""
    checked, bad = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    rc = load().swmi_pk_selftest_product_mad(ctypes.byref(checked), ctypes.byref(bad))
    if rc < 0:
        raise SwmiError(rc, "swmi_pk_selftest_product_mad failed (HIP error or no device)")
    return checked.value, bad.value


def selftest_max3_negative():
    """(comparisons made, mismatches) of swmi_pk_selftest_max3_negative: v_pk_maximum3_f16 drops a finite negative half against
    every pair of non-negative ones in [0, 0x7C00)^2."""
    checked, bad = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    rc = load().swmi_pk_selftest_max3_negative(ctypes.byref(checked), ctypes.byref(bad))
    if rc < 0:
        raise SwmiError(rc, "swmi_pk_selftest_max3_negative failed (HIP error or no device)")
    return checked.value, bad.value
