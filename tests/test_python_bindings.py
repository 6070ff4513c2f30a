"""What swmi/__init__.py's table-aligner wrappers hand to the C ABI, with no device and no library call: swmi._lib is swapped
for a stand-in that records (symbol, arguments) and returns 0.  Seven families with one shape per call (local_align,
local_align_affine, semiglobal_full, semiglobal_full_affine, local_full, local_full_affine, global_full), each with a host
wrapper, a _device wrapper, a timer and a *_slices_for, and the ragged wrappers of both local aligners: the symbol, every
argument by value and position, the result arrays' shapes and dtypes, and the ValueError and SwmiError cases.  The module's
public functions and their signatures are pinned by tests/python_api.txt."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT

N, LEN1, LEN2 = 3, 5, 7
SM = (np.arange(16) * 3 - 20).astype(np.int8)       # 16 distinct entries; int8 and contiguous, so it is passed where it lies
LINEAR, AFFINE = (3,), (4, 2)
D1, D2, DSC, DEN, DMV, DCT, STREAM = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 7   # "device pointers" and a stream


class Recorder:
    """Stands in for the loaded library: every symbol is a function that records its call and returns 0."""

    def __init__(self, on_call=None):
        self.calls, self.on_call = [], on_call

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if self.on_call:
                self.on_call(name, args)        # (while the wrapper's arrays are alive)
            return 0
        return entry


@pytest.fixture
def rec(swmi_mod, monkeypatch):
    r = Recorder()
    monkeypatch.setattr(swmi_mod, "_lib", r)
    assert swmi_mod.load() is r
    return r


class Family:
    def __init__(self, host, timer, slices, gap, len2=LEN2, ends=4, words=2, move_words=None, masks=(None,)):
        self.host, self.device, self.timer, self.slices = host, host + "_device", timer, slices
        self.gap, self.len2, self.ends, self.words, self.masks = gap, len2, ends, words, masks
        self.fixed = len2 == 128                # the (len1, 128) aligners take no len2
        self.move_words = move_words

    def shape(self, seq1s, seq2s):
        return (seq1s, LEN1, seq2s, N) if self.fixed else (seq1s, LEN1, seq2s, self.len2, N)

    def sizes(self):
        return (N, LEN1) if self.fixed else (N, LEN1, self.len2)

    def __repr__(self):
        return self.host


# words: (((len1 + len2 + 31) // 32) + 1) & ~1 = 6 for 5 + 128 and 2 for 5 + 7
FAMILIES = [
    Family("local_align", "local_time_device", "local_slices_for", LINEAR, len2=128, words=6, move_words="local_move_words"),
    Family("local_align_affine", "local_affine_time_device", "local_affine_slices_for", AFFINE, len2=128, words=6,
           move_words="local_move_words"),
    Family("semiglobal_full", "semiglobal_full_time_device", "semiglobal_full_slices_for", LINEAR, ends=2,
           move_words="semiglobal_full_move_words"),
    Family("semiglobal_full_affine", "semiglobal_full_affine_time_device", "semiglobal_full_affine_slices_for", AFFINE, ends=2,
           move_words="semiglobal_full_move_words"),
    Family("local_full", "local_full_time_device", "local_full_slices_for", LINEAR, move_words="local_full_move_words"),
    Family("local_full_affine", "local_full_affine_time_device", "local_full_affine_slices_for", AFFINE,
           move_words="local_full_move_words"),
    Family("global_full", "global_full_time_device", "global_full_slices_for", LINEAR, move_words="global_full_move_words",
           masks=(None, 10, -3)),               # 10 = ENDS_FIT; None = the default, ENDS_GLOBAL
]


def _seqs(fam):
    rng = np.random.default_rng(1)
    return rng.integers(0, 4, (N, LEN1), dtype=np.uint8), rng.integers(0, 4, (N, fam.len2), dtype=np.uint8)


def _mask_args(fam, mask):
    """(what the Python wrapper is given, what the C entry must get) for the free-ends mask."""
    if fam.host != "global_full":
        return (), ()
    return (() if mask is None else (mask,)), ((0 if mask is None else mask) & 0xFFFFFFFF,)


def _ptr(array):
    return None if array is None else array.ctypes.data


@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("fam", FAMILIES, ids=repr)
def test_host_wrapper(swmi_mod, rec, fam, traceback):
    assert swmi_mod.ENDS_FIT == 10
    a, b = _seqs(fam)
    for mask in fam.masks:
        given, passed = _mask_args(fam, mask)
        del rec.calls[:]
        scores, ends, moves, counts = getattr(swmi_mod, fam.host)(a, b, SM, *fam.gap, *given, traceback=traceback)
        assert rec.calls == [("swmi_" + fam.host, fam.shape(a.ctypes.data, b.ctypes.data) + (SM.ctypes.data,) + fam.gap + passed
                              + (scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(counts)))]
        assert (scores.shape, scores.dtype) == ((N,), np.int32) and (ends.shape, ends.dtype) == ((N, fam.ends), np.int32)
        if traceback:
            assert getattr(swmi_mod, fam.move_words)(*((LEN1,) if fam.fixed else (LEN1, fam.len2))) == fam.words
            assert (moves.shape, moves.dtype) == ((N, fam.words), np.uint64) and (counts.shape, counts.dtype) == ((N,), np.uint32)
        else:
            assert moves is None and counts is None and rec.calls[0][1][-2:] == (None, None)


@pytest.mark.parametrize("fam", FAMILIES, ids=repr)
def test_device_wrapper_and_timer(swmi_mod, rec, fam):
    for mask in fam.masks:
        given, passed = _mask_args(fam, mask)
        if fam.host == "global_full" and mask is None:
            given = (swmi_mod.ENDS_GLOBAL,)     # (free_ends has no default in the device wrappers)
        for d_moves, d_counts in ((DMV, DCT), (None, None)):
            want = fam.shape(D1, D2) + (SM.ctypes.data,) + fam.gap + passed + (DSC, DEN, d_moves, d_counts, STREAM)
            tail = () if d_moves is None else (d_moves, d_counts)
            del rec.calls[:]
            assert getattr(swmi_mod, fam.device)(*fam.shape(D1, D2), SM, *fam.gap, *given, DSC, DEN, *tail, stream=STREAM) is None
            assert rec.calls == [("swmi_" + fam.device, want)]
            del rec.calls[:]
            ms = getattr(swmi_mod, fam.timer)(*fam.shape(D1, D2), SM, *fam.gap, *given, DSC, DEN, *tail, stream=STREAM, iters=2)
            assert type(ms) is float and ms == 0.0
            (name, args), = rec.calls
            assert name == "swmi_" + fam.timer and args[:-1] == want + (2,)
            assert type(args[-1]).__name__ == "CArgObject"          # byref(c_float): where the library writes the time
    del rec.calls[:]
    getattr(swmi_mod, fam.device)(*fam.shape(D1, D2), SM, *fam.gap, *_mask_args(fam, 10)[0], DSC, DEN)
    getattr(swmi_mod, fam.timer)(*fam.shape(D1, D2), SM, *fam.gap, *_mask_args(fam, 10)[0], DSC, DEN)
    assert rec.calls[0][1][-3:] == (None, None, 0) and rec.calls[1][1][-5:-1] == (None, None, 0, 10)   # stream 0, iters 10


def _check_slices(rec, symbol, head):
    """The two-call idiom: (.., NULL, 0) for the count, then (.., buffer, count)."""
    (n1, a1), (n2, a2) = rec.calls
    assert n1 == n2 == symbol and a1 == head + (None, 0)
    assert a2[:-2] == head and a2[-1] == 0 and isinstance(a2[-2], ctypes.Array) and a2[-2]._type_ is ctypes.c_size_t


@pytest.mark.parametrize("fam", FAMILIES, ids=repr)
def test_slices_for(swmi_mod, rec, fam):
    for kwargs, flag in (({}, 1), ({"traceback": False}, 0)):
        del rec.calls[:]
        assert getattr(swmi_mod, fam.slices)(*fam.sizes(), **kwargs) == []
        _check_slices(rec, "swmi_" + fam.slices, fam.sizes() + (flag,))


@pytest.mark.parametrize("fam", FAMILIES, ids=repr)
def test_value_errors(swmi_mod, rec, fam):
    a, b = _seqs(fam)
    host = getattr(swmi_mod, fam.host)
    with pytest.raises(ValueError, match=r"must be \(n, len1\)"):
        host(a[0], b, SM, *fam.gap)                                 # a 1-D input
    with pytest.raises(ValueError, match="different numbers of sequences"):
        host(a, b[:2], SM, *fam.gap)
    if fam.fixed:
        with pytest.raises(ValueError, match="last dimension must be 128"):
            host(a, b[:, :127], SM, *fam.gap)
    else:
        with pytest.raises(ValueError, match=r"must be \(n, len1\) and \(n, len2\)"):
            host(a, b[0], SM, *fam.gap)
    with pytest.raises(ValueError, match="score_matrix must have 16 entries"):
        host(a, b, SM[:15], *fam.gap)
    assert rec.calls == []


RAGGED = [("local_align_ragged", LINEAR, False), ("local_align_affine_ragged", AFFINE, False),
          ("local_full_ragged", LINEAR, True), ("local_full_affine_ragged", AFFINE, True)]


def _ragged_inputs(both, lens1, lens2):
    """(seq1s, seq2s, offsets1, offsets2); seq2s is (n, 128) for the aligners that are ragged on one side."""
    rng = np.random.default_rng(2)
    seq1s = [rng.integers(0, 4, k, dtype=np.uint8) for k in lens1]
    seq2s = [rng.integers(0, 4, k, dtype=np.uint8) for k in lens2] if both else rng.integers(0, 4, (len(lens1), 128), dtype=np.uint8)
    return seq1s, seq2s, np.cumsum((0,) + lens1, dtype=np.uint64), np.cumsum((0,) + lens2, dtype=np.uint64)


@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("lens1, lens2", [((0, 5, 2), (0, 0, 3)), ((0, 0, 0), (0, 0, 0))])
@pytest.mark.parametrize("name, gap, both", RAGGED)
def test_ragged_host_wrapper(swmi_mod, monkeypatch, name, gap, both, lens1, lens2, traceback):
    seq1s, seq2s, off1, off2 = _ragged_inputs(both, lens1, lens2)
    seen = {}

    def peek(symbol, args):                     # the staged layouts, read while the wrapper holds them
        if symbol == "swmi_" + name:
            sides = ((args[0], args[1], off1), (args[2], args[3], off2)) if both else ((args[0], args[1], off1),)
            for k, (cat, off, want) in enumerate(sides):
                seen["off%d" % k] = list((ctypes.c_uint64 * (N + 1)).from_address(off))
                assert cat                      # never NULL: an all-empty side gets a valid pointer
                seen["cat%d" % k] = bytes((ctypes.c_uint8 * int(want[-1])).from_address(cat))
    rec = Recorder(peek)
    monkeypatch.setattr(swmi_mod, "_lib", rec)
    scores, ends, moves, move_offsets, steps = getattr(swmi_mod, name)(seq1s, seq2s, SM, *gap, traceback=traceback)
    assert seen["off0"] == list(off1) and seen["cat0"] == np.concatenate(seq1s).tobytes()
    if both:
        assert seen["off1"] == list(off2) and seen["cat1"] == np.concatenate(seq2s).tobytes()
    layout = "swmi_local_full_ragged_move_offsets" if both else "swmi_local_ragged_move_offsets"
    assert [c[0] for c in rec.calls] == ([layout] if traceback else []) + ["swmi_" + name]
    args = rec.calls[-1][1]
    head = 5 if both else 4
    assert args[head - 1] == N and (both or args[2] == seq2s.ctypes.data)
    assert args[head:] == (SM.ctypes.data,) + gap + (scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps))
    assert (scores.shape, scores.dtype) == ((N,), np.int32) and (ends.shape, ends.dtype) == ((N, 4), np.int32)
    if traceback:
        offsets_call = rec.calls[0][1]
        assert offsets_call[-2:] == (N, move_offsets.ctypes.data) and (move_offsets.shape, move_offsets.dtype) == ((N + 1,), np.uint64)
        assert moves.ndim == 1 and moves.dtype == np.uint64 and moves.size == int(move_offsets[-1])
        assert (steps.shape, steps.dtype) == ((N,), np.uint32)
    else:
        assert moves is None and move_offsets is None and steps is None and args[-2:] == (None, None)


@pytest.mark.parametrize("name, gap, both", RAGGED)
def test_ragged_pair_form_is_passed_where_it_lies(swmi_mod, rec, name, gap, both):
    """A (concatenated uint8, offsets uint64) pair is not copied: the C entry gets the caller's addresses."""
    seq1s, seq2s, off1, off2 = _ragged_inputs(both, (0, 5, 2), (0, 0, 3))
    cat1 = np.concatenate(seq1s)
    if both:
        cat2 = np.concatenate(seq2s)
        getattr(swmi_mod, name)((cat1, off1), (cat2, off2), SM, *gap, traceback=False)
        assert rec.calls[0][1][:5] == (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, N)
    else:
        getattr(swmi_mod, name)((cat1, off1), seq2s, SM, *gap, traceback=False)
        assert rec.calls[0][1][:4] == (cat1.ctypes.data, off1.ctypes.data, seq2s.ctypes.data, N)
    with pytest.raises(ValueError, match="different numbers of sequences"):
        getattr(swmi_mod, name)((cat1, off1), seq2s[:2], SM, *gap)
    assert len(rec.calls) == 1


@pytest.mark.parametrize("name, gap, both", RAGGED)
def test_ragged_device_wrapper(swmi_mod, rec, name, gap, both):
    _, _, off1, off2 = _ragged_inputs(both, (0, 5, 2), (0, 0, 3))
    shape_in = (D1, off1, D2, off2) if both else (D1, off1, D2)
    shape_out = (D1, off1.ctypes.data, D2, off2.ctypes.data, N) if both else (D1, off1.ctypes.data, D2, N)
    for d_moves, d_steps in ((DMV, DCT), (None, None)):
        tail = () if d_moves is None else (d_moves, d_steps)
        del rec.calls[:]
        assert getattr(swmi_mod, name + "_device")(*shape_in, SM, *gap, DSC, DEN, *tail, stream=STREAM) is None
        assert rec.calls == [("swmi_" + name + "_device", shape_out + (SM.ctypes.data,) + gap + (DSC, DEN, d_moves, d_steps, STREAM))]


@pytest.mark.parametrize("both", [False, True])
def test_ragged_slices_for(swmi_mod, rec, both):
    _, _, off1, off2 = _ragged_inputs(both, (0, 5, 2), (0, 0, 3))
    name = "local_full_ragged_slices_for" if both else "local_ragged_slices_for"
    offsets = (off1, off2) if both else (off1,)
    for kwargs, flags in (({}, (0, 1)), ({"affine": True, "traceback": False}, (1, 0))):
        del rec.calls[:]
        assert getattr(swmi_mod, name)(*offsets, **kwargs) == []
        _check_slices(rec, "swmi_" + name, tuple(o.ctypes.data for o in offsets) + (N,) + flags)


def _affine_calls(swmi_mod, gap_open, gap_extend):
    """The 13 wrappers that take (gap_open, gap_extend), each as a call with these two."""
    a = np.zeros((N, LEN1), np.uint8)
    b, b128 = np.zeros((N, LEN2), np.uint8), np.zeros((N, 128), np.uint8)
    _, _, off1, off2 = _ragged_inputs(True, (0, 5, 2), (0, 0, 3))
    gaps = (gap_open, gap_extend)
    calls = {}
    for stem, timer, seq2s, shape in (("local_align_affine", "local_affine_time_device", b128, (D1, LEN1, D2, N)),
                                      ("semiglobal_full_affine", "semiglobal_full_affine_time_device", b, (D1, LEN1, D2, LEN2, N)),
                                      ("local_full_affine", "local_full_affine_time_device", b, (D1, LEN1, D2, LEN2, N))):
        calls[stem] = lambda f=getattr(swmi_mod, stem), s=seq2s: f(a, s, SM, *gaps)
        calls[stem + "_device"] = lambda f=getattr(swmi_mod, stem + "_device"), s=shape: f(*s, SM, *gaps, DSC, DEN)
        calls[timer] = lambda f=getattr(swmi_mod, timer), s=shape: f(*s, SM, *gaps, DSC, DEN)
    calls["local_align_affine_ragged"] = lambda: swmi_mod.local_align_affine_ragged([a[0]] * N, b128, SM, *gaps)
    calls["local_align_affine_ragged_device"] = lambda: swmi_mod.local_align_affine_ragged_device(D1, off1, D2, SM, *gaps, DSC, DEN)
    calls["local_full_affine_ragged"] = lambda: swmi_mod.local_full_affine_ragged([a[0]] * N, [b[0]] * N, SM, *gaps)
    calls["local_full_affine_ragged_device"] = lambda: swmi_mod.local_full_affine_ragged_device(D1, off1, D2, off2, SM, *gaps, DSC, DEN)
    assert len(calls) == 13
    return calls


def test_affine_gaps_outside_int32_are_refused(swmi_mod, rec):
    """ctypes would wrap a gap that does not fit a C int (2**32 + 1 would align as gap 1): every affine wrapper raises
    SwmiError(ERR_DOMAIN) before any call; the ends of the int32 range still reach the library, whose own check applies."""
    for bad in (2**31, -2**31 - 1):
        for gaps in ((bad, 2), (4, bad)):
            for name, call in _affine_calls(swmi_mod, *gaps).items():
                with pytest.raises(swmi_mod.SwmiError) as e:
                    call()
                assert e.value.code == swmi_mod.ERR_DOMAIN, name
                assert rec.calls == [], name
    for name, call in _affine_calls(swmi_mod, 2**31 - 1, -2**31).items():
        del rec.calls[:]
        call()
        args = rec.calls[-1][1]
        at = args.index(SM.ctypes.data)
        assert args[at + 1: at + 3] == (2**31 - 1, -2**31), name


def _public_functions(module):
    return sorted((n, f) for n, f in vars(module).items() if inspect.isfunction(f) and not n.startswith("_"))


def _api_snapshot():
    return open(os.path.join(ROOT, "tests", "python_api.txt")).read().splitlines()


def test_public_api_is_unchanged(swmi_mod):
    """tests/python_api.txt: one line per public function of swmi, name(signature), written from the module as it stood
    before the table-aligner wrappers were folded onto shared helpers, by

        python -c "import inspect, swmi; print('\\n'.join(sorted('%s%s' % (n, inspect.signature(f)) for n, f in
            vars(swmi).items() if inspect.isfunction(f) and not n.startswith('_'))))" > tests/python_api.txt

    The module defines exactly these: every name, parameter name, order and default."""
    want = _api_snapshot()
    assert len(want) == 94
    assert ["%s%s" % (n, inspect.signature(f)) for n, f in _public_functions(swmi_mod)] == want


def test_every_public_function_has_a_docstring(swmi_mod):
    """Every function tests/python_api.txt lists is an explicit def with a docstring of its own (help() and the documents rely
    on it).  Before the fold 18 of the 94 had none (init, num_gpus, shutdown, last_error, set_schedule, get_schedule,
    device_info, score_batch, score_one_vs_many, score_batch_packed, score_banded_affine_device,
    semiglobal_xdrop_moves_device, semiglobal_xdrop_device, unpack, score_one_vs_many_device, generate_pairs_device,
    generate_pairs_host, time_batch_device); every table-aligner wrapper had one."""
    functions = dict(_public_functions(swmi_mod))
    for line in _api_snapshot():
        name = line.split("(")[0]
        assert (functions[name].__doc__ or "").strip(), name
        assert functions[name].__module__ == swmi_mod.__name__ and functions[name].__name__ == name
