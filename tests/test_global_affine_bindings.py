"""What swmi/global_affine.py hands to the C ABI, with no device and no library call: swmi._lib is swapped for the stand-in of
test_python_bindings.py, which records (symbol, arguments) and returns 0.  The host wrapper, the _device wrapper, the timer
and *_slices_for: the symbol, every argument by value and position, the result arrays' shapes and dtypes, the ValueError and
SwmiError cases; and the package's own top-level functions are still the pinned 94 of tests/python_api.txt."""
import inspect

import numpy as np
import pytest

from test_python_bindings import D1, D2, DCT, DEN, DMV, DSC, LEN1, LEN2, N, SM, STREAM, Recorder, _api_snapshot, _check_slices, _ptr, \
    _public_functions

OPEN, EXTEND = 4, 2
WORDS = 2               # (((5 + 7 + 31) // 32) + 1) & ~1
MASKS = ((None, 0), (10, 10), (15, 15), (-3, (-3) & 0xFFFFFFFF))     # (given, what the C entry must get); None: the default


@pytest.fixture
def rec(swmi_mod, monkeypatch):
    r = Recorder()
    monkeypatch.setattr(swmi_mod, "_lib", r)
    assert swmi_mod.load() is r
    return r


def _seqs():
    rng = np.random.default_rng(1)
    return rng.integers(0, 4, (N, LEN1), dtype=np.uint8), rng.integers(0, 4, (N, LEN2), dtype=np.uint8)


@pytest.mark.parametrize("traceback", [True, False])
def test_host_wrapper(swmi_mod, rec, traceback):
    a, b = _seqs()
    for given, passed in MASKS:
        del rec.calls[:]
        extra = () if given is None else (given,)
        scores, ends, moves, steps = swmi_mod.global_affine.global_full_affine(a, b, SM, OPEN, EXTEND, *extra, traceback=traceback)
        assert rec.calls == [("swmi_global_full_affine", (a.ctypes.data, LEN1, b.ctypes.data, LEN2, N, SM.ctypes.data, OPEN, EXTEND, passed,
                                                          scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps)))]
        assert (scores.shape, scores.dtype) == ((N,), np.int32) and (ends.shape, ends.dtype) == ((N, 4), np.int32)
        if traceback:
            assert swmi_mod.global_full_move_words(LEN1, LEN2) == WORDS
            assert (moves.shape, moves.dtype) == ((N, WORDS), np.uint64) and (steps.shape, steps.dtype) == ((N,), np.uint32)
        else:
            assert moves is None and steps is None and rec.calls[0][1][-2:] == (None, None)
    del rec.calls[:]
    swmi_mod.global_affine.global_full_affine(a, b, SM, gap_extend=EXTEND, gap_open=OPEN, free_ends=swmi_mod.ENDS_FIT)   # by keyword
    assert rec.calls[0][1][6:9] == (OPEN, EXTEND, 10)


def test_device_wrapper_and_timer(swmi_mod, rec):
    ga = swmi_mod.global_affine
    shape = (D1, LEN1, D2, LEN2, N)
    for given, passed in MASKS:
        mask = swmi_mod.ENDS_GLOBAL if given is None else given       # (free_ends has no default in the device wrappers)
        for d_moves, d_steps in ((DMV, DCT), (None, None)):
            want = shape + (SM.ctypes.data, OPEN, EXTEND, passed, DSC, DEN, d_moves, d_steps, STREAM)
            tail = () if d_moves is None else (d_moves, d_steps)
            del rec.calls[:]
            assert ga.global_full_affine_device(*shape, SM, OPEN, EXTEND, mask, DSC, DEN, *tail, stream=STREAM) is None
            assert rec.calls == [("swmi_global_full_affine_device", want)]
            del rec.calls[:]
            ms = ga.global_full_affine_time_device(*shape, SM, OPEN, EXTEND, mask, DSC, DEN, *tail, stream=STREAM, iters=2)
            assert type(ms) is float and ms == 0.0
            (name, args), = rec.calls
            assert name == "swmi_global_full_affine_time_device" and args[:-1] == want + (2,)
            assert type(args[-1]).__name__ == "CArgObject"          # byref(c_float): where the library writes the time
    del rec.calls[:]
    ga.global_full_affine_device(*shape, SM, OPEN, EXTEND, 10, DSC, DEN)
    ga.global_full_affine_time_device(*shape, SM, OPEN, EXTEND, 10, DSC, DEN)
    assert rec.calls[0][1][-3:] == (None, None, 0) and rec.calls[1][1][-5:-1] == (None, None, 0, 10)   # stream 0, iters 10


def test_slices_for_and_release(swmi_mod, rec):
    ga = swmi_mod.global_affine
    for kwargs, flag in (({}, 1), ({"traceback": False}, 0)):
        del rec.calls[:]
        assert ga.global_full_affine_slices_for(N, LEN1, LEN2, **kwargs) == []
        _check_slices(rec, "swmi_global_full_affine_slices_for", (N, LEN1, LEN2, flag))
    del rec.calls[:]
    assert ga.global_full_affine_release_workspaces() is None
    assert rec.calls == [("swmi_global_full_affine_release_workspaces", ())]


def test_value_errors(swmi_mod, rec):
    a, b = _seqs()
    host = swmi_mod.global_affine.global_full_affine
    with pytest.raises(ValueError, match=r"must be \(n, len1\) and \(n, len2\)"):
        host(a[0], b, SM, OPEN, EXTEND)                             # a 1-D input
    with pytest.raises(ValueError, match=r"must be \(n, len1\) and \(n, len2\)"):
        host(a, b[0], SM, OPEN, EXTEND)
    with pytest.raises(ValueError, match="different numbers of sequences"):
        host(a, b[:2], SM, OPEN, EXTEND)
    with pytest.raises(ValueError, match="score_matrix must have 16 entries"):
        host(a, b, SM[:15], OPEN, EXTEND)
    assert rec.calls == []


def test_gaps_outside_int32_are_refused(swmi_mod, rec):
    """ctypes would wrap a gap that does not fit a C int: every wrapper raises SwmiError(ERR_DOMAIN) before any call; the ends
    of the int32 range still reach the library, whose own check applies."""
    ga = swmi_mod.global_affine
    a, b = _seqs()
    shape = (D1, LEN1, D2, LEN2, N)

    def calls(go, ge):
        return {"host": lambda: ga.global_full_affine(a, b, SM, go, ge),
                "device": lambda: ga.global_full_affine_device(*shape, SM, go, ge, 0, DSC, DEN),
                "timer": lambda: ga.global_full_affine_time_device(*shape, SM, go, ge, 0, DSC, DEN)}
    for bad in (2**31, -2**31 - 1):
        for gaps in ((bad, 2), (4, bad)):
            for name, call in calls(*gaps).items():
                with pytest.raises(swmi_mod.SwmiError) as e:
                    call()
                assert e.value.code == swmi_mod.ERR_DOMAIN, name
                assert rec.calls == [], name
    for name, call in calls(2**31 - 1, -2**31).items():
        del rec.calls[:]
        call()
        args = rec.calls[-1][1]
        at = args.index(SM.ctypes.data)
        assert args[at + 1: at + 3] == (2**31 - 1, -2**31), name


def test_the_package_namespace_is_unchanged(swmi_mod):
    """The submodule is imported as a module: none of its functions is a top-level function of swmi, whose list is still the
    pinned one."""
    want = _api_snapshot()
    assert len(want) == 94
    assert ["%s%s" % (n, inspect.signature(f)) for n, f in _public_functions(swmi_mod)] == want
    assert inspect.ismodule(swmi_mod.global_affine)
    for name, f in vars(swmi_mod.global_affine).items():
        if inspect.isfunction(f) and not name.startswith("_") and f.__module__ == swmi_mod.global_affine.__name__:
            assert not hasattr(swmi_mod, name), name
            assert (f.__doc__ or "").strip(), name
