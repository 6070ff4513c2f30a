"""ctypes binding of libswmi.so (include/swmi.h) -- the Python-side mirror used by tests/ and bench.py.

The scoring entry points keep the reference's argument meaning (source.cpp:462-466):
``score_pair(seq1, seq2, score_matrix, gap_penalty) -> int`` with 128-byte sequences, a 16-entry int8
matrix indexed ``seq1_base * 4 + seq2_base`` and a non-negative gap penalty.  Nothing here computes
scores on the CPU: every call goes through the C ABI into the gfx950 kernels and raises ``SwmiError``
when the library or a usable device is missing.
"""
import ctypes
import os

import numpy as np

SEQ_LEN = 128
PACKED_LEN = 32

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWMI_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libswmi.so"))   # SWMI_LIB: A/B builds (tools/)

OK = 0
ERR_NOT_INITIALIZED = -1
ERR_NO_DEVICE = -2
ERR_UNSUPPORTED_ARCH = -3
ERR_INVALID_ARGUMENT = -4
ERR_DOMAIN = -5
ERR_ALIGNMENT = -6
ERR_HIP = -7
ERR_QUEUE_FULL = -8

NO_GAP_FOLD = 1
USE_I16 = 2
USE_LUT = 4
NO_PACKED = 8


class SwmiError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("swmi error %d: %s" % (code, message))
        self.code = code


class DeviceInfo(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("compute_units", ctypes.c_int), ("clock_khz", ctypes.c_int),
                ("wavefront_size", ctypes.c_int), ("hbm_bytes", ctypes.c_size_t), ("arch", ctypes.c_char * 64),
                ("name", ctypes.c_char * 128)]


_lib = None


def load():
    """dlopen libswmi.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SwmiError(ERR_NOT_INITIALIZED, "%s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, u64, i8 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int8
    lib.swmi_last_error.restype = ctypes.c_char_p
    lib.swmi_init.argtypes = [ctypes.c_int]
    lib.swmi_init_all.argtypes = [ctypes.c_int]
    lib.swmi_init_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.swmi_use_gpu.argtypes = [ctypes.c_int]
    lib.swmi_shard_bounds.argtypes = [sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.swmi_score_batch_multi.argtypes = [vp, vp, sz, vp, i8, vp]
    lib.swmi_score_batch_packed_multi.argtypes = [vp, vp, sz, vp, i8, vp]
    lib.swmi_sharded_create.argtypes = [sz, ctypes.c_int, ctypes.POINTER(vp)]
    lib.swmi_sharded_destroy.argtypes = [vp]
    lib.swmi_sharded_generate.argtypes = [vp, u64, u64]
    lib.swmi_sharded_upload.argtypes = [vp, vp, vp]
    lib.swmi_sharded_score.argtypes = [vp, vp, i8, ctypes.c_int]
    lib.swmi_sharded_wait.argtypes = [vp]
    lib.swmi_sharded_scores_host.argtypes = [vp, vp]
    lib.swmi_sharded_gathered_device.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp)]
    lib.swmi_sharded_gather_backend.argtypes = [vp]
    lib.swmi_sharded_gathered_host.argtypes = [vp, ctypes.c_int, vp]
    lib.swmi_sharded_time.argtypes = [vp, vp, i8, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                      ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
    lib.swmi_host_granules.argtypes = [sz, vp, sz]
    lib.swmi_host_granules.restype = sz
    lib.swmi_host_granules_for.argtypes = [sz, ctypes.c_int, vp, sz]
    lib.swmi_host_granules_for.restype = sz
    lib.swmi_selftest_pk_max3.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
    lib.swmi_sharded_gather_note.argtypes = [vp, ctypes.c_char_p, sz]
    lib.swmi_rccl_probe.argtypes = [ctypes.c_char_p, sz]
    lib.swmi_score_kernel_for_batch.argtypes = [sz, vp, i8, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int)]
    lib.swmi_banded_affine_kernel_for.argtypes = [ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int)]
    lib.swmi_semiglobal_kernels_for_batch.argtypes = [sz, ctypes.c_char_p, sz, ctypes.c_char_p, sz]
    lib.swmi_score_pair.argtypes = [vp, vp, vp, i8]
    lib.swmi_score_batch.argtypes = [vp, vp, sz, vp, i8, vp]
    lib.swmi_score_batch_device.argtypes = [vp, vp, sz, vp, i8, vp, vp]
    lib.swmi_score_one_vs_many.argtypes = [vp, sz, vp, vp, i8, vp]
    lib.swmi_score_one_vs_many_device.argtypes = [vp, sz, vp, vp, i8, vp, vp]
    lib.swmi_score_batch_packed.argtypes = [vp, vp, sz, vp, i8, vp]
    lib.swmi_score_batch_packed_device.argtypes = [vp, vp, sz, vp, i8, vp, vp]
    lib.swmi_unpack.argtypes = [vp, sz, vp]
    lib.swmi_semiglobal_xdrop.argtypes = [vp, vp, sz, vp, vp, sz, vp]
    lib.swmi_semiglobal_xdrop_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp]
    lib.swmi_semiglobal_xdrop_moves.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.swmi_semiglobal_xdrop_moves_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    lib.swmi_semiglobal_expand_moves.argtypes = [vp, ctypes.c_uint32, vp, sz]
    lib.swmi_semiglobal_long_expand_moves.argtypes = [vp, ctypes.c_uint32, vp, sz]
    lib.swmi_schedule_for_batch.argtypes = [sz]
    lib.swmi_semiglobal_time_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp, ctypes.POINTER(ctypes.c_float)]
    lib.swmi_semiglobal_window_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.swmi_semiglobal_set_exact.argtypes = [ctypes.c_int]
    lib.swmi_score_banded_affine.argtypes = [vp, vp, sz, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp]
    lib.swmi_score_banded_affine_device.argtypes = [vp, vp, sz, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.swmi_queue_create.argtypes = [sz, vp, i8, ctypes.POINTER(vp)]
    lib.swmi_queue_submit.argtypes = [vp, vp, vp]
    lib.swmi_queue_submit.restype = ctypes.c_longlong
    lib.swmi_queue_wait.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    lib.swmi_queue_reset.argtypes = [vp]
    lib.swmi_queue_destroy.argtypes = [vp]
    lib.swmi_set_schedule.argtypes = [ctypes.c_int, ctypes.c_uint]
    lib.swmi_get_schedule.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint)]
    lib.swmi_generate_pairs_device.argtypes = [vp, vp, sz, u64, u64, vp]
    lib.swmi_generate_pairs_host.argtypes = [vp, vp, sz, u64, u64]
    lib.swmi_time_batch_device.argtypes = [vp, vp, sz, vp, i8, vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    lib.swmi_get_device_info.argtypes = [ctypes.POINTER(DeviceInfo)]
    # The table aligners, one row per family: (host entry, its timer, its *_slices_for, <shape>, <gap>).  Every entry takes
    # <shape>, the matrix, <gap>, then scores, ends, moves and counts; <host entry>_device adds the stream, the timer the
    # stream, iters and the result; *_slices_for takes the shape's sizes, traceback, a buffer and its capacity.
    ci, cu, ms = ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_float)
    one_len, two_lens = [vp, sz, vp, sz], [vp, sz, vp, sz, sz]              # seq1s len1 seq2s n | seq1s len1 seq2s len2 n
    ragged1, ragged2 = [vp, vp, vp, sz], [vp, vp, vp, vp, sz]               # seq1s offsets seq2s n | ... seq2s offsets n
    for host, timer, slices, shape, gap in (
            ("swmi_local_align", "swmi_local_time_device", "swmi_local_slices_for", one_len, [i8]),
            ("swmi_local_align_affine", "swmi_local_affine_time_device", "swmi_local_affine_slices_for", one_len, [ci, ci]),
            ("swmi_local_align_ragged", None, None, ragged1, [i8]),
            ("swmi_local_align_affine_ragged", None, None, ragged1, [ci, ci]),
            ("swmi_semiglobal_full", "swmi_semiglobal_full_time_device", "swmi_semiglobal_full_slices_for", two_lens, [i8]),
            ("swmi_semiglobal_full_affine", "swmi_semiglobal_full_affine_time_device", "swmi_semiglobal_full_affine_slices_for",
             two_lens, [ci, ci]),
            ("swmi_local_full", "swmi_local_full_time_device", "swmi_local_full_slices_for", two_lens, [i8]),
            ("swmi_local_full_affine", "swmi_local_full_affine_time_device", "swmi_local_full_affine_slices_for", two_lens, [ci, ci]),
            ("swmi_local_full_ragged", None, None, ragged2, [i8]),
            ("swmi_local_full_affine_ragged", None, None, ragged2, [ci, ci]),
            ("swmi_global_full", "swmi_global_full_time_device", "swmi_global_full_slices_for", two_lens, [i8, cu]),
            ("swmi_global_full_affine", "swmi_global_full_affine_time_device", "swmi_global_full_affine_slices_for", two_lens,
             [ci, ci, cu]),
            ("swmi_global_long", "swmi_global_long_time_device", "swmi_global_long_slices_for", two_lens, [i8, cu]),
            ("swmi_global_long_affine", "swmi_global_long_affine_time_device", "swmi_global_long_affine_slices_for", two_lens,
             [ci, ci, cu]),
            ("swmi_local_long", "swmi_local_long_time_device", "swmi_local_long_slices_for", two_lens, [i8]),
            ("swmi_local_long_affine", "swmi_local_long_affine_time_device", "swmi_local_long_affine_slices_for", two_lens, [ci, ci]),
            ("swmi_semiglobal_long", "swmi_semiglobal_long_time_device", "swmi_semiglobal_long_slices_for", two_lens, [i8]),
            ("swmi_semiglobal_long_affine", "swmi_semiglobal_long_affine_time_device", "swmi_semiglobal_long_affine_slices_for",
             two_lens, [ci, ci]),
            ("swmi_global_full_ragged", None, None, ragged2, [i8, cu]),
            ("swmi_global_full_affine_ragged", None, None, ragged2, [ci, ci, cu]),
            ("swmi_semiglobal_full_ragged", None, None, ragged2, [i8]),
            ("swmi_semiglobal_full_affine_ragged", None, None, ragged2, [ci, ci])):
        args = shape + [vp] + gap + [vp, vp, vp, vp]
        getattr(lib, host).argtypes = args
        getattr(lib, host + "_device").argtypes = args + [vp]
        if timer:
            getattr(lib, timer).argtypes = args + [vp, ci, ms]
            getattr(lib, slices).argtypes = [sz] * shape.count(sz) + [ci, vp, sz]
            getattr(lib, slices).restype = sz
    lib.swmi_local_expand_moves.argtypes = [vp, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, vp, sz]
    lib.swmi_local_full_expand_moves.argtypes = [vp, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, vp, sz]
    lib.swmi_global_long_expand_moves.argtypes = [vp, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, vp, sz]
    lib.swmi_local_long_expand_moves.argtypes = [vp, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, vp, sz]
    lib.swmi_local_ragged_move_offsets.argtypes = [vp, sz, vp]
    lib.swmi_local_ragged_slices_for.argtypes = [vp, sz, ci, ci, vp, sz]
    lib.swmi_local_ragged_slices_for.restype = sz
    lib.swmi_local_full_ragged_move_offsets.argtypes = [vp, vp, sz, vp]
    lib.swmi_local_full_ragged_slices_for.argtypes = [vp, vp, sz, ci, ci, vp, sz]
    lib.swmi_local_full_ragged_slices_for.restype = sz
    lib.swmi_global_full_ragged_slices_for.argtypes = [vp, vp, sz, ci, ci, vp, sz]
    lib.swmi_global_full_ragged_slices_for.restype = sz
    lib.swmi_semiglobal_full_ragged_slices_for.argtypes = [vp, vp, sz, ci, ci, vp, sz]
    lib.swmi_semiglobal_full_ragged_slices_for.restype = sz
    _lib = lib
    return lib


def _check(rc):
    if rc < 0:
        raise SwmiError(rc, load().swmi_last_error().decode())
    return rc


def _u8(a, shape_last):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape[-1] != shape_last:
        raise ValueError("last dimension must be %d" % shape_last)
    return a


def _sm(score_matrix):
    raw = np.asarray(score_matrix).reshape(-1)
    if raw.size != 16:
        raise ValueError("score_matrix must have 16 entries")
    if raw.dtype != np.int8 and (raw.min() < -128 or raw.max() > 127):   # the cast below would wrap silently
        raise SwmiError(ERR_DOMAIN, "score_matrix entries must lie in [-128, 127] (got %d..%d)" % (raw.min(), raw.max()))
    return np.ascontiguousarray(raw, dtype=np.int8)


def _gap(gap_penalty):
    """ctypes converts to int8 without an overflow check (256 would score as gap 0): check the range here, so that the
    C side's domain check sees what the caller meant."""
    g = int(gap_penalty)
    if g < -128 or g > 127:
        raise SwmiError(ERR_DOMAIN, "gap_penalty %d is outside the supported domain [0,127]" % g)
    return g


def _affine_gap(name, value):
    """ctypes converts to int without an overflow check (2**32 + 1 would align as gap 1): check the range here, so that the
    C side's domain check sees what the caller meant."""
    g = int(value)
    if g < -2**31 or g > 2**31 - 1:
        raise SwmiError(ERR_DOMAIN, "%s %d is outside the supported domain [0,127]" % (name, g))
    return g


def match_matrix(match, mismatch):
    """4x4 matrix with `match` on the diagonal and `mismatch` elsewhere (source.cpp:3041-3045)."""
    sm = np.full((4, 4), mismatch, np.int8)
    np.fill_diagonal(sm, match)
    return sm.reshape(16)


def init(device=-1):
    """Bind the process to one GPU (swmi_init): a HIP device ordinal, or -1 for the LOCAL_RANK environment variable if set, else 0."""
    _check(load().swmi_init(device))


def init_all(n_gpus=0):
    """Bind the first n_gpus visible GPUs (0 = all) in this one process; returns the number bound."""
    return _check(load().swmi_init_all(n_gpus))


def init_devices(devices):
    """Bind an explicit device list (a device may repeat: two contexts on one GPU)."""
    arr = (ctypes.c_int * len(devices))(*devices)
    return _check(load().swmi_init_devices(arr, len(devices)))


def num_gpus():
    """The number of bound GPU contexts (0 before init)."""
    return int(load().swmi_num_gpus())


def use_gpu(index):
    """Select which bound GPU this thread's single-GPU calls address."""
    _check(load().swmi_use_gpu(index))


def shutdown():
    """Release every bound GPU context (swmi_shutdown)."""
    _check(load().swmi_shutdown())


def shard_bounds(n, shard, n_shards):
    """[lo, hi) of shard `shard` of `n_shards` -- the C library's rule (swmi_shard_bounds), same as sharding.shard_bounds."""
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    _check(load().swmi_shard_bounds(n, shard, n_shards, ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def last_error():
    """Text of the last error on the calling thread ("" if none)."""
    return load().swmi_last_error().decode()


def set_schedule(lanes_per_alignment=0, flags=0):
    """Lanes per alignment (0 = automatic) and the kernel flags NO_GAP_FOLD, USE_I16, USE_LUT, NO_PACKED (swmi_set_schedule)."""
    _check(load().swmi_set_schedule(lanes_per_alignment, flags))


def get_schedule():
    """(lanes per alignment, flags) as set_schedule left them."""
    lanes, flags = ctypes.c_int(), ctypes.c_uint()
    _check(load().swmi_get_schedule(ctypes.byref(lanes), ctypes.byref(flags)))
    return lanes.value, flags.value


def schedule_for_batch(n):
    """Lanes per alignment a launch of n pairs runs with (what the automatic setting resolves to)."""
    return int(load().swmi_schedule_for_batch(ctypes.c_size_t(n)))


def score_kernel_for_batch(n, score_matrix, gap_penalty, mode=0):
    """(kernel instantiation name, alignments per wavefront) a launch of n pairs with these parameters runs."""
    sm = _sm(score_matrix)
    name, per_wave = ctypes.create_string_buffer(96), ctypes.c_int()
    _check(load().swmi_score_kernel_for_batch(n, sm.ctypes.data, _gap(gap_penalty), mode, name, 96, ctypes.byref(per_wave)))
    return name.value.decode(), per_wave.value


def selftest_pk_max3():
    """(comparisons made, mismatches) of swmi_selftest_pk_max3: v_pk_maximum3_f16 as a packed integer max on [0, 0x7C00)^2."""
    checked, bad = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    _check(load().swmi_selftest_pk_max3(ctypes.byref(checked), ctypes.byref(bad)))
    return checked.value, bad.value


ENTRY_PAIRS, ENTRY_PACKED, ENTRY_ONE_VS_MANY = 0, 1, 2


def host_granules(n, entry=ENTRY_PAIRS):
    """The pipeline granules a host-batch entry cuts n pairs into (needs no device): ENTRY_PAIRS = swmi_score_batch,
    ENTRY_PACKED = swmi_score_batch_packed, ENTRY_ONE_VS_MANY = swmi_score_one_vs_many."""
    count = load().swmi_host_granules_for(n, entry, None, 0)
    buf = (ctypes.c_size_t * max(count, 1))()
    load().swmi_host_granules_for(n, entry, buf, count)
    return [int(buf[k]) for k in range(count)]


def rccl_probe():
    """(usable, reason): whether librccl can be loaded with the entry points the score gather needs (needs no device)."""
    why = ctypes.create_string_buffer(512)
    ok = load().swmi_rccl_probe(why, 512)
    return bool(ok), why.value.decode()


def device_info():
    """The current GPU's swmi_device_info as a dict."""
    info = DeviceInfo()
    _check(load().swmi_get_device_info(ctypes.byref(info)))
    return {"device": info.device, "compute_units": info.compute_units, "clock_khz": info.clock_khz,
            "wavefront_size": info.wavefront_size, "hbm_bytes": info.hbm_bytes, "arch": info.arch.decode(),
            "name": info.name.decode()}


def score_pair(seq1, seq2, score_matrix, gap_penalty):
    """Mirror of SmithWaterman_simd4(seq1, seq2, score_matrix, gap_penalty) (source.cpp:462-466)."""
    a, b, sm = _u8(seq1, SEQ_LEN), _u8(seq2, SEQ_LEN), _sm(score_matrix)
    return _check(load().swmi_score_pair(a.ctypes.data, b.ctypes.data, sm.ctypes.data, _gap(gap_penalty)))


def _scores_out(out, n):
    """The result array of a host entry: a fresh one, or the caller's (C-contiguous int32[n]) -- a fresh array's pages are
    first touched by the copy that fills them, inside the call."""
    if out is None:
        return np.zeros(n, np.int32)
    if not (isinstance(out, np.ndarray) and out.dtype == np.int32 and out.flags.c_contiguous and out.size == n):
        raise ValueError("out must be a C-contiguous int32 array of %d scores" % n)
    return out


def score_batch(seq1s, seq2s, score_matrix, gap_penalty, out=None):
    """scores[k] of n pairs of 128-mers, seq1s and seq2s both (n, 128), from host memory (swmi_score_batch)."""
    a, b, sm = _u8(seq1s, SEQ_LEN), _u8(seq2s, SEQ_LEN), _sm(score_matrix)
    if a.shape != b.shape:
        raise ValueError("seq1s and seq2s must have the same shape")
    n = a.size // SEQ_LEN
    out = _scores_out(out, n)
    _check(load().swmi_score_batch(a.ctypes.data, b.ctypes.data, n, sm.ctypes.data, _gap(gap_penalty), out.ctypes.data))
    return out


def score_batch_multi(seq1s, seq2s, score_matrix, gap_penalty, packed=False):
    """swmi_score_batch[_packed]_multi: the host batch split over every bound GPU (init_all / init_devices)."""
    width = PACKED_LEN if packed else SEQ_LEN
    a, b, sm = _u8(seq1s, width), _u8(seq2s, width), _sm(score_matrix)
    if a.shape != b.shape:
        raise ValueError("seq1s and seq2s must have the same shape")
    n = a.size // width
    out = np.zeros(n, np.int32)
    fn = load().swmi_score_batch_packed_multi if packed else load().swmi_score_batch_multi
    _check(fn(a.ctypes.data, b.ctypes.data, n, sm.ctypes.data, _gap(gap_penalty), out.ctypes.data))
    return out


GATHER_NONE, GATHER_ROOT, GATHER_ALL = 0, 1, 2


class ShardedBatch:
    """A batch whose shards stay resident on the bound GPUs (swmi_sharded_* in include/swmi.h)."""

    def __init__(self, n, packed=False):
        self._b = ctypes.c_void_p()
        self.n = n
        _check(load().swmi_sharded_create(n, 1 if packed else 0, ctypes.byref(self._b)))

    def generate(self, seed, first_pair=0):
        _check(load().swmi_sharded_generate(self._b, seed, first_pair))

    def upload(self, seq1s, seq2s):
        a = np.ascontiguousarray(seq1s, dtype=np.uint8)
        b = np.ascontiguousarray(seq2s, dtype=np.uint8)
        _check(load().swmi_sharded_upload(self._b, a.ctypes.data, b.ctypes.data))

    def score(self, score_matrix, gap_penalty, gather=GATHER_NONE):
        sm = _sm(score_matrix)
        _check(load().swmi_sharded_score(self._b, sm.ctypes.data, _gap(gap_penalty), gather))

    def wait(self):
        _check(load().swmi_sharded_wait(self._b))

    def scores(self):
        out = np.zeros(self.n, np.int32)
        _check(load().swmi_sharded_scores_host(self._b, out.ctypes.data))
        return out

    def gathered_ptr(self, index=0):
        p = ctypes.c_void_p()
        _check(load().swmi_sharded_gathered_device(self._b, index, ctypes.byref(p)))
        return p.value

    def gather_backend(self):
        return {0: "undecided", 1: "p2p", 2: "rccl"}[_check(load().swmi_sharded_gather_backend(self._b))]

    def gather_note(self):
        """Why SWMI_GATHER_ALL runs on peer copies for this batch ("" while RCCL is in use or nothing is decided)."""
        text = ctypes.create_string_buffer(512)
        _check(load().swmi_sharded_gather_note(self._b, text, 512))
        return text.value.decode()

    def gathered(self, index=0):
        """The full score vector GPU `index` holds after a gather, copied to the host."""
        out = np.zeros(self.n, np.int32)
        _check(load().swmi_sharded_gathered_host(self._b, index, out.ctypes.data))
        return out

    def time(self, score_matrix, gap_penalty, gather=GATHER_NONE, iters=10):
        """({"kernel_ms": [...], "gather_ms": [...], "wall_ms": float}) averaged over `iters` back-to-back calls."""
        g = num_gpus()
        k, ga, w = (ctypes.c_float * g)(), (ctypes.c_float * g)(), ctypes.c_double()
        sm = _sm(score_matrix)
        _check(load().swmi_sharded_time(self._b, sm.ctypes.data, _gap(gap_penalty), gather, iters, k, ga, ctypes.byref(w)))
        return {"kernel_ms": [float(x) for x in k], "gather_ms": [float(x) for x in ga], "wall_ms": float(w.value)}

    def close(self):
        if self._b:
            load().swmi_sharded_destroy(self._b)
            self._b = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def score_one_vs_many(seq1s, seq2, score_matrix, gap_penalty, out=None):
    """scores[k] of seq1s[k] against the one seq2, all 128-mers, from host memory (swmi_score_one_vs_many)."""
    a, b, sm = _u8(seq1s, SEQ_LEN), _u8(seq2, SEQ_LEN), _sm(score_matrix)
    n = a.size // SEQ_LEN
    out = _scores_out(out, n)
    _check(load().swmi_score_one_vs_many(a.ctypes.data, n, b.ctypes.data, sm.ctypes.data, _gap(gap_penalty), out.ctypes.data))
    return out


def score_batch_packed(seq1s_packed, seq2s_packed, score_matrix, gap_penalty, out=None):
    """score_batch on 2-bit packed 128-mers, 32 bytes each, as pack() writes them (swmi_score_batch_packed)."""
    a, b, sm = _u8(seq1s_packed, PACKED_LEN), _u8(seq2s_packed, PACKED_LEN), _sm(score_matrix)
    n = a.size // PACKED_LEN
    out = _scores_out(out, n)
    _check(load().swmi_score_batch_packed(a.ctypes.data, b.ctypes.data, n, sm.ctypes.data, _gap(gap_penalty), out.ctypes.data))
    return out


def score_banded_affine(seq1s, seq2s, score_matrix, gap_open, gap_extend):
    """Extension (BASELINE configs[4]): banded (128 diagonals) affine-gap local scores of n pairs of len-mers."""
    a = np.ascontiguousarray(seq1s, dtype=np.uint8)
    b = np.ascontiguousarray(seq2s, dtype=np.uint8)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError("seq1s and seq2s must both be (n, len)")
    n, length = a.shape
    sm = _sm(score_matrix)
    out = np.zeros(n, np.int32)
    _check(load().swmi_score_banded_affine(a.ctypes.data, b.ctypes.data, n, length, sm.ctypes.data, int(gap_open),
                                           int(gap_extend), out.ctypes.data))
    return out


def banded_affine_kernel_for(length, score_matrix, gap_open, gap_extend):
    """(kernel instantiation, alignments per wavefront) a banded-affine launch with these parameters runs (needs no device)."""
    sm = _sm(score_matrix)
    name = ctypes.create_string_buffer(128)
    per = ctypes.c_int()
    _check(load().swmi_banded_affine_kernel_for(int(length), sm.ctypes.data_as(ctypes.c_void_p), int(gap_open), int(gap_extend), name, 128,
                                               ctypes.byref(per)))
    return name.value.decode(), per.value


def score_banded_affine_device(d_seq1s, d_seq2s, n, length, score_matrix, gap_open, gap_extend, d_scores, stream=0):
    """swmi_score_banded_affine_device on device pointers (asynchronous on `stream`)."""
    sm = _sm(score_matrix)
    _check(load().swmi_score_banded_affine_device(d_seq1s, d_seq2s, n, length, sm.ctypes.data, int(gap_open),
                                                  int(gap_extend), d_scores, stream))


SG_LEN = 16384
SG_MAX_TRACEBACK = 32769


def semiglobal_xdrop(seq1s, seq2s, cap=SG_MAX_TRACEBACK):
    """Mirror of SemiGlobal_AdaptiveBanded_XDrop_111_32_70 (source.cpp:1836-1976) for n pairs of 16384-mers.

    Returns (scores[n], list of n (len_k, 2) int32 arrays = the reference's traceback vectors, lengths[n] = the
    reference's .second.size() per alignment, which exceeds len_k only when `cap` cut the traceback short)."""
    a = np.ascontiguousarray(seq1s, dtype=np.uint8).reshape(-1, SG_LEN)
    b = np.ascontiguousarray(seq2s, dtype=np.uint8).reshape(-1, SG_LEN)
    n = a.shape[0]
    scores = np.zeros(n, np.int32)
    lengths = np.zeros(n, np.uint32)
    tb = np.zeros((n, cap, 2), np.int32)
    _check(load().swmi_semiglobal_xdrop(a.ctypes.data, b.ctypes.data, n, scores.ctypes.data, tb.ctypes.data, cap,
                                        lengths.ctypes.data))
    return scores, [tb[k, : min(int(lengths[k]), cap)].copy() for k in range(n)], lengths


SG_MOVE_WORDS = 1040


def semiglobal_xdrop_moves(seq1s, seq2s):
    """The same alignments with the traceback as MOVES (swmi_semiglobal_xdrop_moves): (scores[n], moves[n, SG_MOVE_WORDS] uint64,
    lengths[n]); move t of alignment k = (moves[k, t // 32] >> 2 * (t % 32)) & 3 in walking order (3 diagonal, 2 up, 1 left)."""
    a = np.ascontiguousarray(seq1s, dtype=np.uint8).reshape(-1, SG_LEN)
    b = np.ascontiguousarray(seq2s, dtype=np.uint8).reshape(-1, SG_LEN)
    n = a.shape[0]
    scores = np.zeros(n, np.int32)
    lengths = np.zeros(n, np.uint32)
    moves = np.zeros((n, SG_MOVE_WORDS), np.uint64)
    _check(load().swmi_semiglobal_xdrop_moves(a.ctypes.data, b.ctypes.data, n, scores.ctypes.data, moves.ctypes.data, lengths.ctypes.data))
    return scores, moves, lengths


def semiglobal_expand_moves(moves_row, length, cap=None):
    """One alignment's moves -> the reference's (length, 2) traceback array, on the host (swmi_semiglobal_expand_moves)."""
    row = np.ascontiguousarray(moves_row, dtype=np.uint64)
    cap = int(length) if cap is None else int(cap)
    tb = np.zeros((min(int(length), cap), 2), np.int32)
    _check(load().swmi_semiglobal_expand_moves(row.ctypes.data, int(length), tb.ctypes.data, cap))
    return tb


def semiglobal_xdrop_moves_device(d_seq1s, d_seq2s, n, d_scores, d_moves, d_lengths, stream=0):
    """swmi_semiglobal_xdrop_moves_device on device pointers (asynchronous on `stream`)."""
    _check(load().swmi_semiglobal_xdrop_moves_device(d_seq1s, d_seq2s, n, d_scores, d_moves, d_lengths, stream))


def semiglobal_xdrop_device(d_seq1s, d_seq2s, n, d_scores, d_tracebacks, cap, d_lengths, stream=0):
    """swmi_semiglobal_xdrop_device on device pointers (asynchronous on `stream`)."""
    _check(load().swmi_semiglobal_xdrop_device(d_seq1s, d_seq2s, n, d_scores, d_tracebacks, cap, d_lengths, stream))


def semiglobal_time_device(d_seq1s, d_seq2s, n, d_scores, d_tracebacks, cap, d_lengths, stream=0):
    """(sweep_ms, traceback_ms) of one device call, from HIP events on `stream`."""
    ms = (ctypes.c_float * 2)()
    _check(load().swmi_semiglobal_time_device(d_seq1s, d_seq2s, n, d_scores, d_tracebacks, cap, d_lengths, stream, ms))
    return float(ms[0]), float(ms[1])


def semiglobal_set_mapping(sweep=-1):
    """Override which semi-global sweep runs (-1 = automatic); see swmi_semiglobal_set_mapping in include/swmi.h."""
    _check(load().swmi_semiglobal_set_mapping(int(sweep)))


def semiglobal_set_exact(exact_only=False):
    """True: the sweeps run the X-drop test in every round (no calm windows); same results, see include/swmi.h."""
    _check(load().swmi_semiglobal_set_exact(1 if exact_only else 0))


def semiglobal_window_stats(stream=0, walk=False):
    """(windows of 8 rounds the sweep wavefronts of the last device call on `stream` ran, how many of them were calm); with
    walk=True also (windows of 16 rounds the traceback wavefronts walked, how many of them twice: a walk left cells 8 .. 23)."""
    c = (ctypes.c_uint64 * 4)()
    _check(load().swmi_semiglobal_window_stats(ctypes.c_void_p(stream), c))
    return (int(c[0]), int(c[1]), int(c[2]), int(c[3])) if walk else (int(c[0]), int(c[1]))


def semiglobal_kernels_for_batch(n):
    """(sweep kernel name, traceback kernel name) a call with n alignments runs on the current GPU."""
    a, b = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
    _check(load().swmi_semiglobal_kernels_for_batch(n, a, 96, b, 96))
    return a.value.decode(), b.value.decode()


LOCAL_SEQ2_LEN = 128
LOCAL_MAX_LEN = 16384


# The table aligners (local, exact semi-global, any-length local and global; linear and affine gaps; one shape or ragged) share
# one argument order in include/swmi.h:
#     entry(<shape>, matrix, <gap>, scores, ends, moves, counts[, stream[, iters, &ms]])
# A public wrapper below names its C entry, builds <shape> and hands (matrix, <gap>) over as `params`; these helpers do the rest.

def _linear(score_matrix, gap_penalty, *mask):
    """`params` of a linear-gap aligner, checked: (matrix, gap) and, for the global aligner, the free-ends mask."""
    return (_sm(score_matrix), _gap(gap_penalty)) + mask


def _affine(score_matrix, gap_open, gap_extend):
    """`params` of an affine aligner, checked: (matrix, gap_open, gap_extend)."""
    return _sm(score_matrix), _affine_gap("gap_open", gap_open), _affine_gap("gap_extend", gap_extend)


def _call(entry, shape, params, *tail):
    """entry(*shape, matrix address, *gap, *tail), checked.  `params` carries the matrix itself, so that it outlives the call."""
    return _check(entry(*shape, params[0].ctypes.data, *params[1:], *tail))


def _ptr(array):
    return None if array is None else array.ctypes.data


def _table_align(entry, shape, params, n, ends_width, moves_shape, traceback):
    """A host entry on fresh result arrays: (scores[n] int32, ends[n, ends_width] int32, moves[moves_shape] uint64, counts[n]
    uint32 = steps or lengths); traceback=False: ends-only (moves and counts are None, in the call and in the result)."""
    scores = np.zeros(n, np.int32)
    ends = np.zeros((n, ends_width), np.int32)
    moves = np.zeros(moves_shape, np.uint64) if traceback else None
    counts = np.zeros(n, np.uint32) if traceback else None
    _call(entry, shape, params, scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(counts))
    return scores, ends, moves, counts


def _table_time(entry, shape, params, *tail, iters):
    """Average ms of a *_time_device entry; tail = (d_scores, d_ends, d_moves, d_counts, stream)."""
    ms = ctypes.c_float()
    _call(entry, shape, params, *tail, int(iters), ctypes.byref(ms))
    return float(ms.value)


def _slices(entry, *args):
    """A *_slices_for entry's list: one call for the count, one to fill a buffer of that many."""
    count = entry(*args, None, 0)
    buf = (ctypes.c_size_t * max(count, 1))()
    entry(*args, buf, count)
    return [int(buf[k]) for k in range(count)]


def _expand(entry, moves_row, steps, end_i, end_j, cap):
    row = np.ascontiguousarray(moves_row, dtype=np.uint64)
    count = int(steps) + 1 if cap is None else min(int(steps) + 1, int(cap))
    pos = np.zeros((count, 2), np.int32)
    _check(entry(row.ctypes.data, int(steps), int(end_i), int(end_j), pos.ctypes.data, count))
    return pos


def _move_words(len1, len2):
    return (((int(len1) + int(len2) + 31) // 32) + 1) & ~1


def _pair_batch_128(seq1s, seq2s):
    """(a, b, n, len1) of a batch of one seq1 length against 128-mers."""
    a = np.ascontiguousarray(seq1s, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("seq1s must be (n, len1)")
    b = _u8(seq2s, LOCAL_SEQ2_LEN).reshape(-1, LOCAL_SEQ2_LEN)
    n, len1 = a.shape
    if b.shape[0] != n:
        raise ValueError("seq1s and seq2s hold different numbers of sequences")
    return a, b, n, len1


def _pair_batch(seq1s, seq2s):
    """(a, b, n, len1, len2) of a batch of one (len1, len2)."""
    a = np.ascontiguousarray(seq1s, dtype=np.uint8)
    b = np.ascontiguousarray(seq2s, dtype=np.uint8)
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError("seq1s and seq2s must be (n, len1) and (n, len2)")
    n, len1 = a.shape
    if b.shape[0] != n:
        raise ValueError("seq1s and seq2s hold different numbers of sequences")
    return a, b, n, len1, b.shape[1]


def local_move_words(len1):
    """64-bit words of moves per alignment of swmi_local_align (SWMI_LOCAL_MOVE_WORDS)."""
    return _move_words(len1, LOCAL_SEQ2_LEN)


def local_align(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """Local alignment with end cell, start cell and traceback (swmi_local_align): the reference's SmithWaterman_111_long
    (source.cpp:1526-1576) for n pairs, any int8 matrix and gap.  seq1s: (n, len1) bases, seq2s: (n, 128).

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves[n, local_move_words(len1)] uint64,
    steps[n] uint32); move t of alignment k = (moves[k, t // 32] >> 2 * (t % 32)) & 3 in walking order from the end cell
    (3 diagonal, 2 up, 1 left).  traceback=False: ends-only (moves and steps are None, the start cell is (-1, -1))."""
    a, b, n, len1 = _pair_batch_128(seq1s, seq2s)
    return _table_align(load().swmi_local_align, (a.ctypes.data, len1, b.ctypes.data, n), _linear(score_matrix, gap_penalty), n, 4,
                        (n, local_move_words(max(len1, 1))), traceback)


def local_align_device(d_seq1s, len1, d_seq2s, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None, d_steps=None,
                       stream=0):
    """swmi_local_align_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_local_align_device, (d_seq1s, len1, d_seq2s, n), _linear(score_matrix, gap_penalty), d_scores, d_ends,
          d_moves, d_steps, stream)


def local_time_device(d_seq1s, len1, d_seq2s, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None, d_steps=None,
                      stream=0, iters=10):
    """Average ms of one swmi_local_align_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_local_time_device, (d_seq1s, len1, d_seq2s, n), _linear(score_matrix, gap_penalty), d_scores,
                       d_ends, d_moves, d_steps, stream, iters=iters)


def local_expand_moves(moves_row, steps, end_i, end_j, cap=None):
    """One alignment's moves -> the reference's (steps + 1, 2) int32 list of (i, j) from the start cell to the end cell."""
    return _expand(load().swmi_local_expand_moves, moves_row, steps, end_i, end_j, cap)


def local_slices_for(n, len1, traceback=True):
    """The slices swmi_local_align cuts n alignments into (needs no device)."""
    return _slices(load().swmi_local_slices_for, n, len1, 1 if traceback else 0)


def local_align_affine(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """Local alignment with affine gaps, end cell, start cell and traceback (swmi_local_align_affine): a gap of length k costs
    gap_open + (k-1) gap_extend.  Same arguments and return value as local_align, with (gap_open, gap_extend) for the gap."""
    a, b, n, len1 = _pair_batch_128(seq1s, seq2s)
    return _table_align(load().swmi_local_align_affine, (a.ctypes.data, len1, b.ctypes.data, n),
                        _affine(score_matrix, gap_open, gap_extend), n, 4, (n, local_move_words(max(len1, 1))), traceback)


def local_align_affine_device(d_seq1s, len1, d_seq2s, n, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                              d_steps=None, stream=0):
    """swmi_local_align_affine_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_local_align_affine_device, (d_seq1s, len1, d_seq2s, n), _affine(score_matrix, gap_open, gap_extend), d_scores,
          d_ends, d_moves, d_steps, stream)


def local_affine_time_device(d_seq1s, len1, d_seq2s, n, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                             d_steps=None, stream=0, iters=10):
    """Average ms of one swmi_local_align_affine_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_local_affine_time_device, (d_seq1s, len1, d_seq2s, n), _affine(score_matrix, gap_open, gap_extend),
                       d_scores, d_ends, d_moves, d_steps, stream, iters=iters)


def local_affine_slices_for(n, len1, traceback=True):
    """The slices swmi_local_align_affine cuts n alignments into (needs no device)."""
    return _slices(load().swmi_local_affine_slices_for, n, len1, 1 if traceback else 0)


def _ragged_seq1s(seq1s):
    """(concatenated uint8, offsets uint64[n + 1]) from a list of 1-D arrays or from such a pair."""
    if isinstance(seq1s, tuple):
        cat, off = seq1s
        cat = np.ascontiguousarray(cat, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
        if len(off) < 1:
            raise ValueError("offsets must hold n + 1 entries")
        if int(off[-1]) > len(cat):
            raise ValueError("offsets point past the concatenated seq1s")
        return cat, off
    parts = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1) for x in seq1s]
    off = np.zeros(len(parts) + 1, np.uint64)
    if parts:
        off[1:] = np.cumsum([len(x) for x in parts], dtype=np.uint64)
    cat = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return cat, off


def local_ragged_move_offsets(seq1_offsets):
    """move_offsets[n + 1] of a ragged batch (swmi_local_ragged_move_offsets; needs no device)."""
    off = np.ascontiguousarray(seq1_offsets, dtype=np.uint64).reshape(-1)
    out = np.zeros(len(off), np.uint64)
    _check(load().swmi_local_ragged_move_offsets(off.ctypes.data, len(off) - 1, out.ctypes.data))
    return out


def local_ragged_slices_for(seq1_offsets, affine=False, traceback=True):
    """The slices a ragged call cuts its batch into (swmi_local_ragged_slices_for; needs no device)."""
    off = np.ascontiguousarray(seq1_offsets, dtype=np.uint64).reshape(-1)
    return _slices(load().swmi_local_ragged_slices_for, off.ctypes.data, len(off) - 1, 1 if affine else 0, 1 if traceback else 0)


def _ragged_align(entry, shape, params, n, move_offsets, traceback):
    """_table_align with the moves flat, alignment k's at move_offsets[k]: (scores, ends, moves, move_offsets, steps)."""
    scores, ends, moves, steps = _table_align(entry, shape, params, n, 4, int(move_offsets[-1]) if traceback else 0, traceback)
    return scores, ends, moves, move_offsets, steps


def _ragged_call(entry, seq1s, seq2s, params, traceback):
    cat, off = _ragged_seq1s(seq1s)
    n = len(off) - 1
    b = _u8(seq2s, LOCAL_SEQ2_LEN).reshape(-1, LOCAL_SEQ2_LEN) if n else np.zeros((0, LOCAL_SEQ2_LEN), np.uint8)
    if b.shape[0] != n:
        raise ValueError("seq1s and seq2s hold different numbers of sequences")
    mo = local_ragged_move_offsets(off) if traceback else None
    if len(cat) == 0:
        cat = np.zeros(16, np.uint8)        # every seq1 is empty: a valid pointer the library never reads
    return _ragged_align(entry, (cat.ctypes.data, off.ctypes.data, b.ctypes.data, n), params, n, mo, traceback)


def local_align_ragged(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """swmi_local_align_ragged: local_align with a seq1 length of its own (0 .. 16384) per alignment.  seq1s: a list of 1-D
    uint8 arrays, or a (concatenated, offsets[n + 1]) pair; seq2s: (n, 128).

    Returns (scores[n] int32, ends[n, 4] int32, moves uint64 (flat: alignment k's at move_offsets[k] ..), move_offsets[n + 1],
    steps[n] uint32); traceback=False: moves, move_offsets and steps are None."""
    return _ragged_call(load().swmi_local_align_ragged, seq1s, seq2s, _linear(score_matrix, gap_penalty), traceback)


def local_align_affine_ragged(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi_local_align_affine_ragged: local_align_affine on a ragged batch; arguments and result as local_align_ragged."""
    return _ragged_call(load().swmi_local_align_affine_ragged, seq1s, seq2s, _affine(score_matrix, gap_open, gap_extend), traceback)


def _ragged_device(entry, d_seq1s, seq1_offsets, d_seq2s, params, *tail):
    off = np.ascontiguousarray(seq1_offsets, dtype=np.uint64).reshape(-1)
    _call(entry, (d_seq1s, off.ctypes.data, d_seq2s, len(off) - 1), params, *tail)


def local_align_ragged_device(d_seq1s, seq1_offsets, d_seq2s, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None,
                              d_steps=None, stream=0):
    """swmi_local_align_ragged_device: device pointers, seq1_offsets a host array of n + 1 (asynchronous on `stream`)."""
    _ragged_device(load().swmi_local_align_ragged_device, d_seq1s, seq1_offsets, d_seq2s, _linear(score_matrix, gap_penalty),
                   d_scores, d_ends, d_moves, d_steps, stream)


def local_align_affine_ragged_device(d_seq1s, seq1_offsets, d_seq2s, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                                     d_moves=None, d_steps=None, stream=0):
    """swmi_local_align_affine_ragged_device: as local_align_ragged_device with (gap_open, gap_extend)."""
    _ragged_device(load().swmi_local_align_affine_ragged_device, d_seq1s, seq1_offsets, d_seq2s,
                   _affine(score_matrix, gap_open, gap_extend), d_scores, d_ends, d_moves, d_steps, stream)


SGFULL_MAX_LEN = 16384


def semiglobal_full_move_words(len1, len2):
    """64-bit words of moves per alignment of swmi_semiglobal_full (SWMI_SGFULL_MOVE_WORDS)."""
    return _move_words(len1, len2)


def semiglobal_full(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """Exact semi-global alignment with traceback (swmi_semiglobal_full): the reference's SemiGlobal_111
    (source.cpp:1776-1834) for n pairs, any lengths in [1, 16384] (one (len1, len2) per call), any int8 matrix and gap.
    seq1s: (n, len1) bases, seq2s: (n, len2).

    Returns (scores[n] int32, ends[n, 2] int32 = the best cell, moves[n, semiglobal_full_move_words(len1, len2)] uint64,
    lengths[n] uint32); move t of alignment k = (moves[k, t // 32] >> 2 * (t % 32)) & 3 in walking order from the best
    cell to (0,0) (3 diagonal, 2 up, 1 left), lengths = steps + 1; semiglobal_expand_moves(moves[k], lengths[k]) gives the
    reference's list.  traceback=False: ends-only (moves and lengths are None)."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_semiglobal_full, (a.ctypes.data, len1, b.ctypes.data, len2, n), _linear(score_matrix, gap_penalty),
                        n, 2, (n, _move_words(len1, len2)), traceback)


def semiglobal_full_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None,
                           d_lengths=None, stream=0):
    """swmi_semiglobal_full_device on device pointers (asynchronous on `stream`); d_moves = d_lengths = None: ends-only."""
    _call(load().swmi_semiglobal_full_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty), d_scores,
          d_ends, d_moves, d_lengths, stream)


def semiglobal_full_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None,
                                d_lengths=None, stream=0, iters=10):
    """Average ms of one swmi_semiglobal_full_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_semiglobal_full_time_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty),
                       d_scores, d_ends, d_moves, d_lengths, stream, iters=iters)


def semiglobal_full_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_semiglobal_full cuts n alignments into (needs no device)."""
    return _slices(load().swmi_semiglobal_full_slices_for, n, len1, len2, 1 if traceback else 0)


def semiglobal_full_release_workspaces():
    """Free the exact semi-global aligner's device buffers on the current GPU."""
    _check(load().swmi_semiglobal_full_release_workspaces())


def semiglobal_full_affine(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """Exact semi-global alignment with affine gaps and traceback (swmi_semiglobal_full_affine): semiglobal_full with a gap of
    length k costing gap_open + (k-1) gap_extend.  Same arguments and return value as semiglobal_full, with (gap_open,
    gap_extend) for the gap."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_semiglobal_full_affine, (a.ctypes.data, len1, b.ctypes.data, len2, n),
                        _affine(score_matrix, gap_open, gap_extend), n, 2, (n, _move_words(len1, len2)), traceback)


def semiglobal_full_affine_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                                  d_moves=None, d_lengths=None, stream=0):
    """swmi_semiglobal_full_affine_device on device pointers (asynchronous on `stream`); d_moves = d_lengths = None: ends-only."""
    _call(load().swmi_semiglobal_full_affine_device, (d_seq1s, len1, d_seq2s, len2, n), _affine(score_matrix, gap_open, gap_extend),
          d_scores, d_ends, d_moves, d_lengths, stream)


def semiglobal_full_affine_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                                       d_moves=None, d_lengths=None, stream=0, iters=10):
    """Average ms of one swmi_semiglobal_full_affine_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_semiglobal_full_affine_time_device, (d_seq1s, len1, d_seq2s, len2, n),
                       _affine(score_matrix, gap_open, gap_extend), d_scores, d_ends, d_moves, d_lengths, stream, iters=iters)


def semiglobal_full_affine_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_semiglobal_full_affine cuts n alignments into (needs no device)."""
    return _slices(load().swmi_semiglobal_full_affine_slices_for, n, len1, len2, 1 if traceback else 0)


def semiglobal_full_affine_release_workspaces():
    """Free the affine exact semi-global aligner's device buffers on the current GPU."""
    _check(load().swmi_semiglobal_full_affine_release_workspaces())


LOCAL_FULL_MAX_LEN = 16384


def local_full_move_words(len1, len2):
    """64-bit words of moves per alignment of swmi_local_full (SWMI_LOCAL_FULL_MOVE_WORDS)."""
    return _move_words(len1, len2)


def local_full(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """Local alignment of two sequences of any length with end cell, start cell and traceback (swmi_local_full): local_align
    with a seq2 of any length in [1, 16384] (one (len1, len2) per call), any int8 matrix and gap.  seq1s: (n, len1) bases,
    seq2s: (n, len2).  For len2 == 128 local_align gives the same results faster.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves[n, local_full_move_words(len1, len2)]
    uint64, steps[n] uint32); move t of alignment k = (moves[k, t // 32] >> 2 * (t % 32)) & 3 in walking order from the end
    cell (3 diagonal, 2 up, 1 left); local_full_expand_moves(moves[k], steps[k], end_i, end_j) gives the reference's list.
    traceback=False: ends-only (moves and steps are None, the start cell is (-1, -1))."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_local_full, (a.ctypes.data, len1, b.ctypes.data, len2, n), _linear(score_matrix, gap_penalty),
                        n, 4, (n, _move_words(len1, len2)), traceback)


def local_full_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None, d_steps=None,
                      stream=0):
    """swmi_local_full_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_local_full_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty), d_scores, d_ends,
          d_moves, d_steps, stream)


def local_full_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None,
                           d_steps=None, stream=0, iters=10):
    """Average ms of one swmi_local_full_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_local_full_time_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty),
                       d_scores, d_ends, d_moves, d_steps, stream, iters=iters)


def local_full_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_local_full cuts n alignments into (needs no device)."""
    return _slices(load().swmi_local_full_slices_for, n, len1, len2, 1 if traceback else 0)


def local_full_expand_moves(moves_row, steps, end_i, end_j, cap=None):
    """One alignment's moves -> the reference's (steps + 1, 2) int32 list of (i, j) from the start cell to the end cell."""
    return _expand(load().swmi_local_full_expand_moves, moves_row, steps, end_i, end_j, cap)


def local_full_release_workspaces():
    """Free the any-length local aligner's device buffers on the current GPU."""
    _check(load().swmi_local_full_release_workspaces())


GLOBAL_FULL_MAX_LEN = 16384
FREE_BEGIN1, FREE_BEGIN2, FREE_END1, FREE_END2 = 1, 2, 4, 8     # SWMI_FREE_*: which end gaps cost nothing
ENDS_GLOBAL = 0                                                 # Needleman-Wunsch, end to end
ENDS_FIT = FREE_BEGIN2 | FREE_END2                              # all of seq1 against a stretch of seq2
ENDS_OVERLAP = FREE_BEGIN1 | FREE_BEGIN2 | FREE_END1 | FREE_END2


def _free_ends(free_ends):
    """The mask as the C side takes it (an unsigned int; a value outside 0 .. 15, a negative one included, is refused there)."""
    return int(free_ends) & 0xFFFFFFFF


def global_full_move_words(len1, len2):
    """64-bit words of moves per alignment of swmi_global_full (SWMI_GLOBAL_FULL_MOVE_WORDS)."""
    return _move_words(len1, len2)


def global_full(seq1s, seq2s, score_matrix, gap_penalty, free_ends=ENDS_GLOBAL, traceback=True):
    """Global (Needleman-Wunsch) and free-end-gap alignment of two sequences of any length in [1, 16384] with end cell, start
    cell and traceback (swmi_global_full), one (len1, len2) per call, any int8 matrix and gap, no zero floor.  free_ends is a
    mask: FREE_BEGIN1 / FREE_BEGIN2 make column 0 / row 0 hold 0, FREE_END1 / FREE_END2 let the end cell be the best of the
    last column / last row (first in row-major order among equals); ENDS_GLOBAL, ENDS_FIT and ENDS_OVERLAP name the usual
    ones.  seq1s: (n, len1) bases, seq2s: (n, len2).

    Returns (scores[n] int32, which may be negative, ends[n, 4] int32 = (end_i, end_j, start_i, start_j),
    moves[n, global_full_move_words(len1, len2)] uint64, steps[n] uint32); move t of alignment k =
    (moves[k, t // 32] >> 2 * (t % 32)) & 3 in walking order from the end cell (3 diagonal, 2 up, 1 left), forced moves along
    a border that is not free included; local_full_expand_moves(moves[k], steps[k], end_i, end_j) gives the positions from
    the start cell to the end cell.  traceback=False: ends-only (moves and steps are None, the start cell is (-1, -1))."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_global_full, (a.ctypes.data, len1, b.ctypes.data, len2, n),
                        _linear(score_matrix, gap_penalty, _free_ends(free_ends)), n, 4, (n, _move_words(len1, len2)), traceback)


def global_full_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, free_ends, d_scores, d_ends, d_moves=None,
                       d_steps=None, stream=0):
    """swmi_global_full_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_global_full_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty, _free_ends(free_ends)),
          d_scores, d_ends, d_moves, d_steps, stream)


def global_full_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, free_ends, d_scores, d_ends, d_moves=None,
                            d_steps=None, stream=0, iters=10):
    """Average ms of one swmi_global_full_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_global_full_time_device, (d_seq1s, len1, d_seq2s, len2, n),
                       _linear(score_matrix, gap_penalty, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps, stream, iters=iters)


def global_full_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_global_full cuts n alignments into (needs no device)."""
    return _slices(load().swmi_global_full_slices_for, n, len1, len2, 1 if traceback else 0)


def global_full_release_workspaces():
    """Free the global aligner's device buffers on the current GPU."""
    _check(load().swmi_global_full_release_workspaces())


def local_full_affine(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """Local alignment of two sequences of any length with affine gaps, end cell, start cell and traceback
    (swmi_local_full_affine): local_full with a gap of length k costing gap_open + (k-1) gap_extend.  Same arguments and return
    value as local_full, with (gap_open, gap_extend) for the gap; local_full_move_words and local_full_expand_moves apply.
    For len2 == 128 local_align_affine gives the same results faster."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_local_full_affine, (a.ctypes.data, len1, b.ctypes.data, len2, n),
                        _affine(score_matrix, gap_open, gap_extend), n, 4, (n, _move_words(len1, len2)), traceback)


def local_full_affine_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                             d_moves=None, d_steps=None, stream=0):
    """swmi_local_full_affine_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_local_full_affine_device, (d_seq1s, len1, d_seq2s, len2, n), _affine(score_matrix, gap_open, gap_extend),
          d_scores, d_ends, d_moves, d_steps, stream)


def local_full_affine_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                                  d_moves=None, d_steps=None, stream=0, iters=10):
    """Average ms of one swmi_local_full_affine_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_local_full_affine_time_device, (d_seq1s, len1, d_seq2s, len2, n),
                       _affine(score_matrix, gap_open, gap_extend), d_scores, d_ends, d_moves, d_steps, stream, iters=iters)


def local_full_affine_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_local_full_affine cuts n alignments into (needs no device)."""
    return _slices(load().swmi_local_full_affine_slices_for, n, len1, len2, 1 if traceback else 0)


def local_full_affine_release_workspaces():
    """Free the any-length affine local aligner's device buffers on the current GPU."""
    _check(load().swmi_local_full_affine_release_workspaces())


def _ragged_pair(seq1s, seq2s):
    """Both sides of a ragged any-length batch as (concatenated, offsets): each a list of 1-D arrays or such a pair."""
    cat1, off1 = _ragged_seq1s(seq1s)
    cat2, off2 = _ragged_seq1s(seq2s)
    if len(off1) != len(off2):
        raise ValueError("seq1s and seq2s hold different numbers of sequences")
    return cat1, off1, cat2, off2


def _offsets_pair(seq1_offsets, seq2_offsets):
    off1 = np.ascontiguousarray(seq1_offsets, dtype=np.uint64).reshape(-1)
    off2 = np.ascontiguousarray(seq2_offsets, dtype=np.uint64).reshape(-1)
    if len(off1) < 1 or len(off1) != len(off2):
        raise ValueError("seq1_offsets and seq2_offsets must both hold n + 1 entries")
    return off1, off2


def local_full_ragged_move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a ragged any-length batch (swmi_local_full_ragged_move_offsets; needs no device)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    out = np.zeros(len(off1), np.uint64)
    _check(load().swmi_local_full_ragged_move_offsets(off1.ctypes.data, off2.ctypes.data, len(off1) - 1, out.ctypes.data))
    return out


def local_full_ragged_slices_for(seq1_offsets, seq2_offsets, affine=False, traceback=True):
    """The slices a ragged any-length call cuts its batch into (swmi_local_full_ragged_slices_for; needs no device)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    return _slices(load().swmi_local_full_ragged_slices_for, off1.ctypes.data, off2.ctypes.data, len(off1) - 1, 1 if affine else 0,
                   1 if traceback else 0)


def _full_ragged_call(entry, seq1s, seq2s, params, traceback):
    cat1, off1, cat2, off2 = _ragged_pair(seq1s, seq2s)
    n = len(off1) - 1
    mo = local_full_ragged_move_offsets(off1, off2) if traceback else None
    if len(cat1) == 0:
        cat1 = np.zeros(16, np.uint8)       # every seq1 is empty: a valid pointer the library never reads
    if len(cat2) == 0:
        cat2 = np.zeros(16, np.uint8)
    return _ragged_align(entry, (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n), params, n, mo, traceback)


def local_full_ragged(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """swmi_local_full_ragged: local_full with a (len1, len2) of its own (0 .. 16384 each) per alignment.  seq1s and seq2s:
    each a list of 1-D uint8 arrays, or a (concatenated, offsets[n + 1]) pair.

    Returns (scores[n] int32, ends[n, 4] int32, moves uint64 (flat: alignment k's at move_offsets[k] ..), move_offsets[n + 1],
    steps[n] uint32); traceback=False: moves, move_offsets and steps are None."""
    return _full_ragged_call(load().swmi_local_full_ragged, seq1s, seq2s, _linear(score_matrix, gap_penalty), traceback)


def local_full_affine_ragged(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi_local_full_affine_ragged: local_full_affine on a ragged batch; arguments and result as local_full_ragged."""
    return _full_ragged_call(load().swmi_local_full_affine_ragged, seq1s, seq2s, _affine(score_matrix, gap_open, gap_extend), traceback)


def _full_ragged_device(entry, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, params, *tail):
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    _call(entry, (d_seq1s, off1.ctypes.data, d_seq2s, off2.ctypes.data, len(off1) - 1), params, *tail)


def local_full_ragged_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_penalty, d_scores, d_ends,
                             d_moves=None, d_steps=None, stream=0):
    """swmi_local_full_ragged_device: device pointers, both offset arrays host arrays of n + 1 (asynchronous on `stream`)."""
    _full_ragged_device(load().swmi_local_full_ragged_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                        _linear(score_matrix, gap_penalty), d_scores, d_ends, d_moves, d_steps, stream)


def local_full_affine_ragged_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores,
                                    d_ends, d_moves=None, d_steps=None, stream=0):
    """swmi_local_full_affine_ragged_device: as local_full_ragged_device with (gap_open, gap_extend)."""
    _full_ragged_device(load().swmi_local_full_affine_ragged_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                        _affine(score_matrix, gap_open, gap_extend), d_scores, d_ends, d_moves, d_steps, stream)


def unpack(packed):
    """2-bit packed sequences (.., 32) -> bases (.., 128), on the GPU (swmi_unpack; source.cpp:1580-1583)."""
    p = _u8(packed, PACKED_LEN)
    n = p.size // PACKED_LEN
    out = np.zeros((n, SEQ_LEN), np.uint8)
    _check(load().swmi_unpack(p.ctypes.data, n, out.ctypes.data))
    return out.reshape(p.shape[:-1] + (SEQ_LEN,))


def pack(seqs):
    """Host-side inverse of unpack() (source.cpp:1581): base k of byte i at bits 2k..2k+1."""
    s = _u8(seqs, SEQ_LEN).reshape(-1, 32, 4) & 3
    return (s[..., 0] | (s[..., 1] << 2) | (s[..., 2] << 4) | (s[..., 3] << 6)).astype(np.uint8).reshape(seqs.shape[:-1] + (32,))


def score_batch_device(d_seq1s, d_seq2s, n, score_matrix, gap_penalty, d_scores, stream=0, packed=False):
    """Device pointers (ints). Asynchronous on `stream` (a hipStream_t value, 0 = the HIP null stream)."""
    sm = _sm(score_matrix)
    fn = load().swmi_score_batch_packed_device if packed else load().swmi_score_batch_device
    _check(fn(d_seq1s, d_seq2s, n, sm.ctypes.data, _gap(gap_penalty), d_scores, stream))


def score_one_vs_many_device(d_seq1s, n, d_seq2, score_matrix, gap_penalty, d_scores, stream=0):
    """swmi_score_one_vs_many_device on device pointers (asynchronous on `stream`)."""
    sm = _sm(score_matrix)
    _check(load().swmi_score_one_vs_many_device(d_seq1s, n, d_seq2, sm.ctypes.data, _gap(gap_penalty), d_scores, stream))


def generate_pairs_device(d_seq1s, d_seq2s, n, seed, first_pair=0, stream=0):
    """Fill device buffers with pairs first_pair .. first_pair + n of the counter-based generator (asynchronous on `stream`)."""
    _check(load().swmi_generate_pairs_device(d_seq1s, d_seq2s, n, seed, first_pair, stream))


def generate_pairs_host(n, seed, first_pair=0):
    """(seq1s, seq2s), each (n, 128): pairs first_pair .. first_pair + n of the counter-based generator, on the host."""
    a = np.zeros((n, SEQ_LEN), np.uint8)
    b = np.zeros((n, SEQ_LEN), np.uint8)
    _check(load().swmi_generate_pairs_host(a.ctypes.data, b.ctypes.data, n, seed, first_pair))
    return a, b


def time_batch_device(d_seq1s, d_seq2s, n, score_matrix, gap_penalty, d_scores, stream=0, iters=10):
    """Average ms of one batch kernel launch over `iters` back-to-back launches (HIP events on `stream`)."""
    sm = _sm(score_matrix)
    ms = ctypes.c_float()
    _check(load().swmi_time_batch_device(d_seq1s, d_seq2s, n, sm.ctypes.data, _gap(gap_penalty), d_scores, stream, iters,
                                         ctypes.byref(ms)))
    return ms.value


class Queue:
    """Deferred queue behind the per-pair signature (swmi_queue_* in include/swmi.h)."""

    def __init__(self, max_pairs, score_matrix, gap_penalty):
        self._q = ctypes.c_void_p()
        sm = _sm(score_matrix)
        _check(load().swmi_queue_create(max_pairs, sm.ctypes.data, _gap(gap_penalty), ctypes.byref(self._q)))

    def submit(self, seq1, seq2):
        a, b = _u8(seq1, SEQ_LEN), _u8(seq2, SEQ_LEN)
        return _check(load().swmi_queue_submit(self._q, a.ctypes.data, b.ctypes.data))

    def wait(self):
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(load().swmi_queue_wait(self._q, ctypes.byref(ptr), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.int32)
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int32)), shape=(n.value,)).copy()

    def reset(self):
        _check(load().swmi_queue_reset(self._q))

    def close(self):
        if self._q:
            load().swmi_queue_destroy(self._q)
            self._q = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The affine global / free-end-gap aligner's wrappers live in a submodule, swmi.global_affine.<name>: imported as a module
# (last, when every helper it takes from here is defined), its functions stay out of this namespace.
from . import global_affine    # noqa: E402
from . import global_ragged    # noqa: E402  (the global aligners on mixed-shape batches, likewise a submodule)
from . import global_long      # noqa: E402  (the global aligners for lengths up to 65536, likewise a submodule)
from . import local_long       # noqa: E402  (the local aligners for lengths up to 65536, likewise a submodule)
from . import semiglobal_long  # noqa: E402  (the exact semi-global aligners for lengths up to 65536, likewise a submodule)
from . import semiglobal_ragged  # noqa: E402  (the exact semi-global aligners on mixed-shape batches, likewise a submodule)
from . import wide             # noqa: E402  (the wide-alphabet aligners of libswmi_wide.so, likewise a submodule)
from . import wide_long        # noqa: E402  (the wide-alphabet aligners for lengths up to 65536, libswmi_wide_long.so, likewise)
from . import wide_profile     # noqa: E402  (a batch against one position-specific profile, libswmi_wide_profile.so, likewise)
from . import pk_form          # noqa: E402  (the packed scorer's cell-form rule and flag-form self-test, libswmi_pk_form.so, likewise)
from . import banded           # noqa: E402  (banded local alignment with end cells and traceback, libswmi_banded.so, likewise)
from . import banded_global    # noqa: E402  (the band's global, fit, overlap and extension kinds, libswmi_banded_global.so, likewise)
from . import banded_ragged    # noqa: E402  (both banded kinds on mixed-shape batches, libswmi_banded_ragged.so, likewise)
from . import banded_width     # noqa: E402  (the same with a band of 128 .. 1024 diagonals per call, libswmi_banded_width.so, likewise)
from . import banded_long      # noqa: E402  (the same for sequences up to 65536 long, libswmi_banded_long.so, likewise)
