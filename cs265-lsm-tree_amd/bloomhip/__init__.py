"""bloomhip — Python view of the MI355X Bloom-filter engine's C ABI.

Thin ctypes binding of ``include/bloomhip.h`` (``lib/libbloomhip.so``).  It
mirrors the reference's filter surface (jackdent/cs265-lsm-tree
src/bloom_filter.h:6-15) so tests read like the reference's own usage:

    f = BloomFilter(m_bits)         # BloomFilter(long length)   bloom_filter.h:12
    f.set(key)                      # void set(KEY_t)            bloom_filter.cpp:49-53
    f.is_set(key)                   # bool is_set(KEY_t) const   bloom_filter.cpp:55-59

plus the batch calls the GPU needs (``set_batch`` / ``test_batch``) and
``m_bits(max_size, bits_per_entry)`` for Run::Run's sizing (src/run.cpp:13-15).

There is no CPU fallback: if the HIP library is missing this module raises on
import, and every compute call goes through the gfx950 kernels.
"""
from __future__ import annotations

import ctypes
import os
from typing import Sequence

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(os.path.dirname(PKG_DIR), "lib")
# BLOOMHIP_LIB: another build of the same library (tools/ab.sh times two
# builds of the engine against each other in one GPU session).
LIB_PATH = os.environ.get("BLOOMHIP_LIB") or os.path.join(LIB_DIR, "libbloomhip.so")

OK = 0
EIO = -5
ENOMEM = -12
ENODEV = -19
EINVAL = -22
ERANGE = -34

BUILD_AUTO = 0
BUILD_ATOMIC = 1
BUILD_LDS = 2
BUILD_PARTITION = 3
PROBE_AUTO = 0
PROBE_GATHER = 1
PROBE_PARTITION = 2
PROBE_LDS = 3
PROBE_STACKED = 4
STRATEGY_NAMES = {BUILD_AUTO: "auto", BUILD_ATOMIC: "atomic", BUILD_LDS: "lds",
                  BUILD_PARTITION: "partition"}
PROF_SLOTS = 13

# Every symbol include/bloomhip.h and include/bloomhip_workload.h declare.
EXPORTED_SYMBOLS = (
    "bloomhip_abi_version", "bloomhip_kernel_sha", "bloomhip_strerror", "bloomhip_last_error",
    "bloomhip_device_count",
    "bloomhip_m_bits", "bloomhip_create", "bloomhip_destroy", "bloomhip_size",
    "bloomhip_nwords", "bloomhip_device", "bloomhip_device_words", "bloomhip_stream",
    "bloomhip_clear", "bloomhip_set_batch", "bloomhip_test_batch", "bloomhip_set",
    "bloomhip_is_set", "bloomhip_download", "bloomhip_upload", "bloomhip_sync",
    "bloomhip_set_strategy", "bloomhip_set_probe_strategy", "bloomhip_resolve_strategy", "bloomhip_profile_enable",
    "bloomhip_profile_read", "bloomhip_profile_reset", "bloomhip_trim", "bloomhip_host_positions",
    "bloomhip_gen_mt19937", "bloomhip_gen_glibc_rand", "bloomhip_gen_puts",
    "bloomhip_gen_workload", "bloomhip_set_batch_run", "bloomhip_set_run_meta",
    "bloomhip_get_run_meta", "bloomhip_route_gets", "bloomhip_route_gets_packed", "bloomhip_save", "bloomhip_load",
    "bloomhip_build_from_run_file", "bloomhip_compact", "bloomhip_clone", "bloomhip_get_batch",
    "bloomhip_range_batch", "bloomhip_flush_batch", "bloomhip_flush_cuts",
    "bloomhip_tree_plan_host", "bloomhip_tree_create", "bloomhip_tree_destroy",
    "bloomhip_tree_put_batch", "bloomhip_tree_get_batch", "bloomhip_tree_range_batch",
    "bloomhip_tree_shape", "bloomhip_tree_run",
)


class BloomHipError(RuntimeError):
    def __init__(self, status: int, what: str):
        lib = _lib()
        msg = lib.bloomhip_strerror(status).decode()
        detail = lib.bloomhip_last_error().decode()
        super().__init__(f"{what}: {msg} ({status}){' — ' + detail if detail else ''}")
        self.status = status


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        # One HIP runtime per process: torch bundles its own libamdhip64 with the
        # same SONAME as /opt/rocm's.  Loading torch first makes the loader bind
        # this library to torch's copy, so device pointers and streams from
        # torch are valid here; loading ours first would leave torch with a
        # second runtime that cannot see the GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"bloomhip: {LIB_PATH} is missing — build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        P, I, U64, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t
        PU64 = ctypes.POINTER(ctypes.c_uint64)
        sig = {
            "bloomhip_abi_version": (I, []),
            "bloomhip_kernel_sha": (ctypes.c_char_p, []),
            "bloomhip_strerror": (ctypes.c_char_p, [I]),
            "bloomhip_last_error": (ctypes.c_char_p, []),
            "bloomhip_device_count": (I, [ctypes.POINTER(I)]),
            "bloomhip_m_bits": (I, [ctypes.c_int64, ctypes.c_float, PU64]),
            "bloomhip_create": (I, [I, U64, ctypes.POINTER(P)]),
            "bloomhip_destroy": (I, [P]),
            "bloomhip_size": (I, [P, PU64]),
            "bloomhip_nwords": (I, [P, PU64]),
            "bloomhip_device": (I, [P, ctypes.POINTER(I)]),
            "bloomhip_device_words": (I, [P, ctypes.POINTER(P)]),
            "bloomhip_stream": (I, [P, ctypes.POINTER(P)]),
            "bloomhip_clear": (I, [P, P]),
            "bloomhip_set_batch": (I, [P, P, SZ, SZ, I, P]),
            "bloomhip_test_batch": (I, [ctypes.POINTER(P), I, P, SZ, SZ, I, P, I, P]),
            "bloomhip_set": (I, [P, ctypes.c_int32]),
            "bloomhip_is_set": (I, [P, ctypes.c_int32, ctypes.POINTER(I)]),
            "bloomhip_download": (I, [P, P, SZ, P]),
            "bloomhip_upload": (I, [P, P, SZ, P]),
            "bloomhip_sync": (I, [P, P]),
            "bloomhip_set_strategy": (I, [P, I]),
            "bloomhip_set_probe_strategy": (I, [P, I]),
            "bloomhip_resolve_strategy": (I, [P, SZ, ctypes.POINTER(I)]),
            "bloomhip_profile_enable": (I, [P, I]),
            "bloomhip_profile_read": (I, [P, I, ctypes.POINTER(ctypes.c_char_p), PU64,
                                          ctypes.POINTER(ctypes.c_double)]),
            "bloomhip_profile_reset": (I, [P]),
            "bloomhip_trim": (I, []),
            "bloomhip_host_positions": (I, [U64, P, SZ, P]),
            "bloomhip_gen_mt19937": (I, [ctypes.c_uint32, SZ, P]),
            "bloomhip_gen_glibc_rand": (I, [ctypes.c_uint32, SZ, P]),
            "bloomhip_gen_puts": (I, [ctypes.c_uint32, SZ, P, P]),
            "bloomhip_gen_workload": (I, [ctypes.c_uint32, SZ, SZ, ctypes.c_float, ctypes.c_float,
                                          P, P]),
            "bloomhip_set_batch_run": (I, [P, P, SZ, SZ, I, P]),
            "bloomhip_set_run_meta": (I, [P, P, SZ, ctypes.c_int32]),
            "bloomhip_get_run_meta": (I, [P, P, SZ, ctypes.POINTER(SZ),
                                          ctypes.POINTER(ctypes.c_int32)]),
            "bloomhip_route_gets": (I, [ctypes.POINTER(P), I, P, SZ, SZ, I, P, P, P, I, P]),
            "bloomhip_route_gets_packed": (I, [ctypes.POINTER(P), I, P, SZ, SZ, I, P, P, I, P]),
            "bloomhip_get_batch": (I, [ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(SZ), I,
                                       I, P, SZ, SZ, I, P, P, P, I, P]),
            "bloomhip_range_batch": (I, [ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(SZ), I,
                                         I, P, P, SZ, I, P, P, SZ, ctypes.POINTER(SZ), I, I, P]),
            "bloomhip_compact": (I, [ctypes.POINTER(P), P, I, I, I, P, ctypes.POINTER(SZ), I, P,
                                     I, P]),
            "bloomhip_flush_batch": (I, [P, SZ, I, I, P, ctypes.POINTER(SZ), I, P, I, P]),
            "bloomhip_flush_cuts": (I, [P, SZ, I, U64, P, SZ, ctypes.POINTER(SZ), I, P]),
            "bloomhip_tree_plan_host": (I, [P, I, I, U64, P, SZ, ctypes.POINTER(SZ)]),
            "bloomhip_tree_create": (I, [I, U64, I, I, ctypes.c_float, ctypes.POINTER(P)]),
            "bloomhip_tree_destroy": (I, [P]),
            "bloomhip_tree_put_batch": (I, [P, P, SZ, I, ctypes.POINTER(SZ), P]),
            "bloomhip_tree_get_batch": (I, [P, P, SZ, SZ, I, P, P, I, P]),
            "bloomhip_tree_range_batch": (I, [P, P, P, SZ, I, P, P, SZ, ctypes.POINTER(SZ), I, P]),
            "bloomhip_tree_shape": (I, [P, P, PU64]),
            "bloomhip_tree_run": (I, [P, I, I, ctypes.POINTER(P), ctypes.POINTER(P),
                                      ctypes.POINTER(SZ)]),
            "bloomhip_save": (I, [P, ctypes.c_char_p]),
            "bloomhip_clone": (I, [P, I, ctypes.POINTER(P)]),
            "bloomhip_load": (I, [ctypes.c_char_p, I, ctypes.POINTER(P)]),
            "bloomhip_build_from_run_file": (I, [ctypes.c_char_p, U64, ctypes.c_int64,
                                                 ctypes.c_float, I, ctypes.POINTER(P)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def lib():
    return _lib()


def _check(rc: int, what: str) -> None:
    if rc != OK:
        raise BloomHipError(rc, what)


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = _lib().bloomhip_device_count(ctypes.byref(n))
    return n.value if rc == OK else 0


def m_bits(max_size: int, bits_per_entry: float) -> int:
    """Run::Run's filter size (src/run.cpp:13-15): (long)((float)max_size * bpe)."""
    out = ctypes.c_uint64()
    _check(_lib().bloomhip_m_bits(int(max_size), float(bits_per_entry), ctypes.byref(out)),
           "bloomhip_m_bits")
    return out.value


def host_positions(m: int, keys) -> np.ndarray:
    """The engine's own position arithmetic evaluated on the host (self-test hook)."""
    k = np.ascontiguousarray(keys, dtype=np.int32)
    out = np.empty((k.size, 3), dtype=np.uint64)
    _check(_lib().bloomhip_host_positions(m, k.ctypes.data, k.size, out.ctypes.data),
           "bloomhip_host_positions")
    return out


def _nbytes(buf) -> int:
    return buf.nbytes if isinstance(buf, np.ndarray) else buf.numel() * buf.element_size()


def _is_tensor(buf) -> bool:
    # duck-typed so importing this module does not need torch
    return hasattr(buf, "data_ptr") and hasattr(buf, "is_cuda")


def _ptr_of(buf):
    """(address, on_device, keepalive) for a numpy array or a torch tensor."""
    if isinstance(buf, np.ndarray):
        if not buf.flags["C_CONTIGUOUS"]:
            buf = np.ascontiguousarray(buf)
        return buf.ctypes.data, 0, buf
    if _is_tensor(buf):
        if not buf.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return buf.data_ptr(), 1 if buf.is_cuda else 0, buf
    arr = np.ascontiguousarray(buf, dtype=np.int32)
    return arr.ctypes.data, 0, arr


def _keys_ptr(keys, stride: int):
    """_ptr_of for a key vector (KEY_t = int32, src/types.h:4).  The engine
    reads int32 words at `stride` bytes; any other element type would be read
    as the wrong keys, so: numpy integer arrays at stride 4 are converted to
    int32 when every value fits, anything else that is not int32 is refused.
    Strided views (e.g. entry_t runs at stride 8) must be int32 buffers."""
    if isinstance(keys, np.ndarray):
        if keys.dtype != np.int32:
            if stride != 4 or keys.dtype.kind not in "iu":
                raise ValueError(f"keys must be int32 (got {keys.dtype} at stride {stride})")
            if keys.size and (keys.min() < -2**31 or keys.max() > 2**31 - 1):
                raise ValueError("keys out of int32 range")
            keys = keys.astype(np.int32)
    elif _is_tensor(keys):
        if str(keys.dtype) != "torch.int32":
            raise ValueError(f"key tensor must be torch.int32 (got {keys.dtype})")
    return _ptr_of(keys)


def _key_count(keep, stride: int, n):
    avail = _nbytes(keep)
    if n is None:
        return avail // stride
    if n and (n - 1) * stride + 4 > avail:
        raise ValueError(f"{n} keys at stride {stride} need more than the {avail} bytes given")
    return n


def _out_ptr(buf, need_bytes: int, itemsize: int, what: str):
    """_ptr_of for an output buffer: element size and capacity checked."""
    el = buf.itemsize if isinstance(buf, np.ndarray) else buf.element_size()
    if el != itemsize:
        raise ValueError(f"{what}: elements must be {itemsize} bytes (got {el})")
    if _nbytes(buf) < need_bytes:
        raise ValueError(f"{what}: {need_bytes} bytes needed, {_nbytes(buf)} given")
    if isinstance(buf, np.ndarray) and not buf.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{what} must be contiguous")
    return _ptr_of(buf)


def _stream_ptr(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream  # torch.cuda.Stream


class BloomFilter:
    """One device-resident filter (a ``bloomhip_filter`` handle)."""

    def __init__(self, m_bits: int, device: int = 0):
        if m_bits <= 0:
            raise BloomHipError(EINVAL, "BloomFilter(m_bits <= 0)")
        h = ctypes.c_void_p()
        _check(_lib().bloomhip_create(device, m_bits, ctypes.byref(h)), "bloomhip_create")
        self._h = h
        self.m = m_bits
        self.device = device
        n = ctypes.c_uint64()
        _check(_lib().bloomhip_nwords(h, ctypes.byref(n)), "bloomhip_nwords")
        self.nwords = n.value

    @classmethod
    def _adopt(cls, h: ctypes.c_void_p, device: int) -> "BloomFilter":
        self = cls.__new__(cls)
        self._h = h
        self.device = device
        m, n = ctypes.c_uint64(), ctypes.c_uint64()
        _check(_lib().bloomhip_size(h, ctypes.byref(m)), "bloomhip_size")
        _check(_lib().bloomhip_nwords(h, ctypes.byref(n)), "bloomhip_nwords")
        self.m, self.nwords = m.value, n.value
        return self

    @classmethod
    def load(cls, path: str, device: int = 0) -> "BloomFilter":
        """A filter saved with save() (bloomhip_load)."""
        h = ctypes.c_void_p()
        _check(_lib().bloomhip_load(os.fsencode(path), device, ctypes.byref(h)), "bloomhip_load")
        return cls._adopt(h, device)

    @classmethod
    def from_run_file(cls, path: str, n_entries: int, max_size: int, bits_per_entry: float,
                      device: int = 0) -> "BloomFilter":
        """Filter + run metadata rebuilt from a run file of entry_t records
        (bloomhip_build_from_run_file)."""
        h = ctypes.c_void_p()
        _check(_lib().bloomhip_build_from_run_file(os.fsencode(path), n_entries, max_size,
                                                   bits_per_entry, device, ctypes.byref(h)),
               "bloomhip_build_from_run_file")
        return cls._adopt(h, device)

    def clone(self, device: int | None = None) -> "BloomFilter":
        """bloomhip_clone: this filter (bitmap + run metadata) on `device`
        (peer copy over xGMI between GPUs)."""
        dev = self.device if device is None else device
        h = ctypes.c_void_p()
        _check(_lib().bloomhip_clone(self._h, dev, ctypes.byref(h)), "bloomhip_clone")
        return BloomFilter._adopt(h, dev)

    def save(self, path: str) -> None:
        _check(_lib().bloomhip_save(self._h, os.fsencode(path)), "bloomhip_save")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            if not getattr(self, "_borrowed", False):  # a view of a tree's run is the tree's
                _lib().bloomhip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # --- reference surface ------------------------------------------------
    def set(self, key: int) -> None:
        _check(_lib().bloomhip_set(self._h, int(key)), "bloomhip_set")

    def is_set(self, key: int) -> bool:
        hit = ctypes.c_int(0)
        _check(_lib().bloomhip_is_set(self._h, int(key), ctypes.byref(hit)), "bloomhip_is_set")
        return bool(hit.value)

    # --- batches ----------------------------------------------------------
    def set_batch(self, keys, n: int | None = None, stride: int = 4, stream=None) -> None:
        ptr, on_dev, keep = _keys_ptr(keys, stride)
        n = _key_count(keep, stride, n)
        _check(_lib().bloomhip_set_batch(self._h, ptr, n, stride, on_dev, _stream_ptr(stream)),
               "bloomhip_set_batch")

    def set_batch_run(self, keys, n: int | None = None, stride: int = 4, stream=None) -> None:
        """set() of a whole run written in this key order, plus its fence
        pointers and max key (Run::put, src/run.cpp:158-174)."""
        ptr, on_dev, keep = _keys_ptr(keys, stride)
        n = _key_count(keep, stride, n)
        _check(_lib().bloomhip_set_batch_run(self._h, ptr, n, stride, on_dev,
                                             _stream_ptr(stream)), "bloomhip_set_batch_run")

    def set_run_meta(self, fences, max_key: int) -> None:
        f = np.ascontiguousarray(fences, dtype=np.int32)
        _check(_lib().bloomhip_set_run_meta(self._h, f.ctypes.data if f.size else None, f.size,
                                            max_key), "bloomhip_set_run_meta")

    def run_meta(self):
        """(fences int32[], max_key)."""
        nf, mk = ctypes.c_size_t(), ctypes.c_int32()
        _check(_lib().bloomhip_get_run_meta(self._h, None, 0, ctypes.byref(nf), None),
               "bloomhip_get_run_meta")
        out = np.empty(nf.value, dtype=np.int32)
        _check(_lib().bloomhip_get_run_meta(self._h, out.ctypes.data if out.size else None,
                                            out.size, ctypes.byref(nf), ctypes.byref(mk)),
               "bloomhip_get_run_meta")
        return out, mk.value

    def clear(self, stream=None) -> None:
        _check(_lib().bloomhip_clear(self._h, _stream_ptr(stream)), "bloomhip_clear")

    def words(self) -> np.ndarray:
        """Bitmap as ceil(m/64) uint64 blocks (dynamic_bitset layout)."""
        out = np.empty(self.nwords, dtype=np.uint64)
        _check(_lib().bloomhip_download(self._h, out.ctypes.data, out.size, None),
               "bloomhip_download")
        return out

    def load_words(self, words: np.ndarray) -> None:
        w = np.ascontiguousarray(words, dtype=np.uint64)
        _check(_lib().bloomhip_upload(self._h, w.ctypes.data, w.size, None), "bloomhip_upload")

    def device_words_ptr(self) -> int:
        p = ctypes.c_void_p()
        _check(_lib().bloomhip_device_words(self._h, ctypes.byref(p)), "bloomhip_device_words")
        return p.value

    def stream_ptr(self) -> int:
        p = ctypes.c_void_p()
        _check(_lib().bloomhip_stream(self._h, ctypes.byref(p)), "bloomhip_stream")
        return p.value or 0

    def sync(self, stream=None) -> None:
        _check(_lib().bloomhip_sync(self._h, _stream_ptr(stream)), "bloomhip_sync")

    def set_strategy(self, strategy: int) -> None:
        _check(_lib().bloomhip_set_strategy(self._h, strategy), "bloomhip_set_strategy")

    def set_probe_strategy(self, strategy: int) -> None:
        _check(_lib().bloomhip_set_probe_strategy(self._h, strategy), "bloomhip_set_probe_strategy")

    def resolve_strategy(self, n: int) -> int:
        s = ctypes.c_int()
        _check(_lib().bloomhip_resolve_strategy(self._h, n, ctypes.byref(s)),
               "bloomhip_resolve_strategy")
        return s.value

    # --- profiling ----------------------------------------------------------
    def profile(self, enable: bool = True) -> None:
        _check(_lib().bloomhip_profile_enable(self._h, 1 if enable else 0), "profile_enable")

    def profile_reset(self) -> None:
        _check(_lib().bloomhip_profile_reset(self._h), "profile_reset")

    def profile_read(self) -> dict:
        res = {}
        for slot in range(PROF_SLOTS):
            name = ctypes.c_char_p()
            launches = ctypes.c_uint64()
            ms = ctypes.c_double()
            _check(_lib().bloomhip_profile_read(self._h, slot, ctypes.byref(name),
                                                ctypes.byref(launches), ctypes.byref(ms)),
                   "profile_read")
            if launches.value:
                res[name.value.decode()] = {"launches": launches.value, "ms": ms.value}
        return res


def test_batch(filters: Sequence[BloomFilter], keys, n: int | None = None, stride: int = 4,
               out=None, stream=None):
    """is_set of every key against each filter.  Returns (or fills) a packed
    [nf, ceil(n/64)] uint64 array: bit i%64 of row j word i/64 = filters[j].is_set(key i)."""
    ptr, on_dev, keep = _keys_ptr(keys, stride)
    n = _key_count(keep, stride, n)
    nf = len(filters)
    nw = (n + 63) // 64
    if out is None:
        out = np.zeros((nf, nw), dtype=np.uint64)
    optr, out_dev, okeep = _out_ptr(out, nf * nw * 8, 8, "out")
    arr = (ctypes.c_void_p * nf)(*[f.handle.value for f in filters])
    _check(_lib().bloomhip_test_batch(arr, nf, ptr, n, stride, on_dev, optr, out_dev,
                                      _stream_ptr(stream)), "bloomhip_test_batch")
    return out


def route_gets(runs: Sequence[BloomFilter], keys, n: int | None = None, stride: int = 4,
               cand=None, first=None, page=None, stream=None):
    """Batched GET routing (bloomhip_route_gets): runs newest first.  Returns
    (cand [nruns, ceil(n/64)] uint64 packed, first int32[n], page int32[n]);
    pass device tensors for all three to keep the outputs on the device."""
    ptr, on_dev, keep = _keys_ptr(keys, stride)
    n = _key_count(keep, stride, n)
    nr = len(runs)
    nw = (n + 63) // 64
    if cand is None and first is None and page is None:
        cand = np.zeros((nr, nw), dtype=np.uint64)
        first = np.empty(n, dtype=np.int32)
        page = np.empty(n, dtype=np.int32)
    need = ((nr * nw * 8, 8, "cand"), (n * 4, 4, "first"), (n * 4, 4, "page"))
    outs = [_out_ptr(x, *nd) if x is not None else (None, None, None)
            for x, nd in zip((cand, first, page), need)]
    devs = {o[1] for o in outs if o[0] is not None}
    if len(devs) > 1:
        raise ValueError("route_gets outputs must be all host or all device buffers")
    out_dev = devs.pop() if devs else 0
    arr = (ctypes.c_void_p * nr)(*[r.handle.value for r in runs])
    _check(_lib().bloomhip_route_gets(arr, nr, ptr, n, stride, on_dev, outs[0][0], outs[1][0],
                                      outs[2][0], out_dev, _stream_ptr(stream)),
           "bloomhip_route_gets")
    return cand, first, page


ROUTE_NONE = 0xFFFFFFFF   # BLOOMHIP_ROUTE_NONE: no candidate run
ROUTE_PAGE_BITS = 28


def route_gets_packed(runs: Sequence[BloomFilter], keys, n: int | None = None, stride: int = 4,
                      cand=None, route=None, stream=None):
    """Batched GET routing with the packed output (bloomhip_route_gets_packed):
    runs newest first (at most 16).  Returns (cand [nruns, ceil(n/64)] uint64
    packed, route uint32[n]) with route[i] = first << 28 | page, or
    ROUTE_NONE; pass device tensors for both to keep them on the device."""
    ptr, on_dev, keep = _keys_ptr(keys, stride)
    n = _key_count(keep, stride, n)
    nr = len(runs)
    nw = (n + 63) // 64
    if cand is None and route is None:
        cand = np.zeros((nr, nw), dtype=np.uint64)
        route = np.empty(n, dtype=np.uint32)
    need = ((nr * nw * 8, 8, "cand"), (n * 4, 4, "route"))
    outs = [_out_ptr(x, *nd) if x is not None else (None, None, None)
            for x, nd in zip((cand, route), need)]
    devs = {o[1] for o in outs if o[0] is not None}
    if len(devs) > 1:
        raise ValueError("route_gets_packed outputs must be all host or all device buffers")
    out_dev = devs.pop() if devs else 0
    arr = (ctypes.c_void_p * nr)(*[r.handle.value for r in runs])
    _check(_lib().bloomhip_route_gets_packed(arr, nr, ptr, n, stride, on_dev, outs[0][0], outs[1][0],
                                             out_dev, _stream_ptr(stream)),
           "bloomhip_route_gets_packed")
    return cand, route


def unpack_route(route):
    """(first, page) int32 arrays from a packed route array, -1 where none."""
    r = np.asarray(route, dtype=np.uint32)
    none = r == ROUTE_NONE
    first = np.where(none, -1, (r >> ROUTE_PAGE_BITS).astype(np.int32)).astype(np.int32)
    page = np.where(none, -1, (r & ((1 << ROUTE_PAGE_BITS) - 1)).astype(np.int32)).astype(np.int32)
    return first, page


VAL_NONE = -2**31  # vals[i] when no run holds key i (= VAL_TOMBSTONE, src/types.h:12)


def get_batch(runs: Sequence[BloomFilter], entries, keys, n: int | None = None, stride: int = 4,
              vals=None, found_run=None, stats=None, stream=None):
    """Batched GET (bloomhip_get_batch): runs newest first, entries[r] run r's
    entry_t records (int32 [n_r, 2] numpy arrays or device tensors, keys
    ascending).  Returns (vals int32[n], found_run int32[n], stats uint64
    [nruns, 2]): the value and the run that holds each key (VAL_NONE and -1
    when none does; a tombstone's value is passed through), and per run its
    page reads and how many of them were false positives.  Outputs are
    allocated on the host when none is given; pass device tensors for those
    wanted to keep them on the device (the others are skipped)."""
    ptr, on_dev, keep = _keys_ptr(keys, stride)
    n = _key_count(keep, stride, n)
    nr = len(runs)
    if len(entries) != nr:
        raise ValueError(f"{nr} runs but {len(entries)} entry arrays")
    for e in entries:  # entry_t {int32 key; int32 val;} (src/types.h:14-22)
        dt = str(e.dtype)
        if dt not in ("int32", "torch.int32") or len(e.shape) != 2 or e.shape[1] != 2:
            raise ValueError(f"entries must be int32 [n, 2] entry_t arrays (got {dt} {tuple(e.shape)})")
    keeps = [_ptr_of(e) for e in entries]
    sizes = [_nbytes(k[2]) // 8 for k in keeps]
    ons = {k[1] for k, sz in zip(keeps, sizes) if sz}  # an empty run has no buffer to place
    if len(ons) > 1:
        raise ValueError("entries must be all host or all device buffers")
    ent_dev = ons.pop() if ons else 0
    if vals is None and found_run is None and stats is None:
        vals = np.empty(n, dtype=np.int32)
        found_run = np.empty(n, dtype=np.int32)
        stats = np.zeros((nr, 2), dtype=np.uint64)
    need = ((n * 4, 4, "vals"), (n * 4, 4, "found_run"), (nr * 16, 8, "stats"))
    outs = [_out_ptr(x, *nd) if x is not None else (None, None, None)
            for x, nd in zip((vals, found_run, stats), need)]
    devs = {o[1] for o in outs if o[0] is not None}
    if len(devs) > 1:
        raise ValueError("get_batch outputs must be all host or all device buffers")
    out_dev = devs.pop() if devs else 0
    harr = (ctypes.c_void_p * max(nr, 1))(*[r.handle.value for r in runs])
    earr = (ctypes.c_void_p * max(nr, 1))(*[k[0] if sz else None for k, sz in zip(keeps, sizes)])
    ns = (ctypes.c_size_t * max(nr, 1))(*sizes)
    _check(_lib().bloomhip_get_batch(harr, earr, ns, nr, ent_dev, ptr, n, stride, on_dev,
                                     outs[0][0], outs[1][0], outs[2][0], out_dev,
                                     _stream_ptr(stream)), "bloomhip_get_batch")
    return vals, found_run, stats


# bloomhip_range_batch's classes (csrc/bloom_range.h kRangeWaveCap,
# kRangeBlockCap): a query with at most RANGE_WAVE_CAP candidate entries (the
# entries of every run inside its bounds) is merged by one wave in LDS, one
# with at most RANGE_BLOCK_CAP by one workgroup; above that it is a compaction.
RANGE_WAVE_CAP = 512
RANGE_BLOCK_CAP = 2048


def range_batch(runs, entries, starts, ends, out=None, offsets=None, device=0, stream=None):
    """Batched RANGE (bloomhip_range_batch): for every query q the entries with
    starts[q] <= key < ends[q] over all runs, keys ascending, the newest run's
    entry of a key winning (runs[0] is the newest) and tombstones dropped.
    runs: BloomFilter handles or None (a run without a handle, such as the
    memtable, is searched whole); entries[r]: run r's entry_t records (int32
    [n_r, 2] numpy arrays or device tensors, keys ascending); starts, ends:
    int32[nq], host or device.  Returns (offsets uint64[nq + 1], out_entries
    int32[total, 2]): query q's answer is out_entries[offsets[q]:offsets[q + 1]].
    With no `out`: one count-only call, an exact allocation (on the device when
    `offsets` is a device tensor), one fill call.  With `out` (int32 [cap, 2],
    host or device like `offsets`): one call, BloomHipError(ERANGE) when it is
    too small; the first `total` rows of `out` are returned."""
    nr = len(runs)
    if len(entries) != nr:
        raise ValueError(f"{nr} runs but {len(entries)} entry arrays")
    for e in entries:  # entry_t {int32 key; int32 val;} (src/types.h:14-22)
        dt = str(e.dtype)
        if dt not in ("int32", "torch.int32") or len(e.shape) != 2 or e.shape[1] != 2:
            raise ValueError(f"entries must be int32 [n, 2] entry_t arrays (got {dt} {tuple(e.shape)})")
    keeps = [_ptr_of(e) for e in entries]
    sizes = [_nbytes(k[2]) // 8 for k in keeps]
    ons = {k[1] for k, sz in zip(keeps, sizes) if sz}  # an empty run has no buffer to place
    if len(ons) > 1:
        raise ValueError("entries must be all host or all device buffers")
    ent_dev = ons.pop() if ons else 0
    sptr, s_dev, skeep = _keys_ptr(starts, 4)
    eptr, e_dev, ekeep = _keys_ptr(ends, 4)
    nq = _nbytes(skeep) // 4
    if _nbytes(ekeep) // 4 != nq:
        raise ValueError("starts and ends must have one length")
    if nq and s_dev != e_dev:
        raise ValueError("starts and ends must be both host or both device buffers")
    if offsets is None:
        if out is not None and _is_tensor(out) and out.is_cuda:
            import torch
            offsets = torch.empty(nq + 1, dtype=torch.int64, device=out.device)
        else:
            offsets = np.empty(nq + 1, dtype=np.uint64)
    optr, out_dev, okeep = _out_ptr(offsets, (nq + 1) * 8, 8, "offsets")
    harr = (ctypes.c_void_p * max(nr, 1))(*[r.handle.value if r is not None else None for r in runs])
    earr = (ctypes.c_void_p * max(nr, 1))(*[k[0] if sz else None for k, sz in zip(keeps, sizes)])
    ns = (ctypes.c_size_t * max(nr, 1))(*sizes)
    total = ctypes.c_size_t()

    def call(buf_ptr, cap):
        return _lib().bloomhip_range_batch(harr, earr, ns, nr, ent_dev, sptr, eptr, nq, s_dev, optr,
                                           buf_ptr, cap, ctypes.byref(total), out_dev, device,
                                           _stream_ptr(stream))

    if out is None:
        _check(call(None, 0), "bloomhip_range_batch")
        if out_dev:
            import torch
            out = torch.empty((total.value, 2), dtype=torch.int32, device=offsets.device)
        else:
            out = np.empty((total.value, 2), dtype=np.int32)
        if total.value == 0:
            return offsets, out
    dt = str(out.dtype)
    if dt not in ("int32", "torch.int32") or len(out.shape) != 2 or out.shape[1] != 2:
        raise ValueError(f"out must be an int32 [capacity, 2] entry_t array (got {dt} {tuple(out.shape)})")
    cap = _nbytes(out) // 8
    bptr, b_dev, bkeep = _out_ptr(out, 0, 4, "out")
    if b_dev != out_dev:
        raise ValueError("offsets and out must be both host or both device buffers")
    _check(call(bptr if cap else None, cap), "bloomhip_range_batch")
    return offsets, out[:total.value]


def compact(runs, drop_tombstones: bool = False, filter: BloomFilter | None = None,
            device: int = 0, out=None, stream=None):
    """Compaction (bloomhip_compact): runs = entry_t arrays (int32 [n, 2] numpy
    arrays or device tensors), newest first.  Returns the merged run (a
    [n_out, 2] int32 array, or the first n_out rows of `out` when given);
    builds `filter` (and its run metadata) from the merged keys when given."""
    nr = len(runs)
    for r in runs:  # entry_t {int32 key; int32 val;} (src/types.h:14-22)
        dt = str(r.dtype)
        if dt not in ("int32", "torch.int32") or len(r.shape) != 2 or r.shape[1] != 2:
            raise ValueError(f"runs must be int32 [n, 2] entry_t arrays (got {dt} {tuple(r.shape)})")
    keeps = [_ptr_of(r) for r in runs]
    ons = {k[1] for k in keeps}
    if len(ons) > 1:
        raise ValueError("runs must be all host or all device buffers")
    on_dev = ons.pop() if ons else 0
    sizes = [_nbytes(k[2]) // 8 for k in keeps]
    total = sum(sizes)
    if out is None:
        out = np.empty((max(total, 1), 2), dtype=np.int32)
    optr, out_dev, okeep = _out_ptr(out, total * 8, 4, "out")
    arr = (ctypes.c_void_p * max(nr, 1))(*[k[0] for k in keeps])
    ns = (ctypes.c_size_t * max(nr, 1))(*sizes)
    n_out = ctypes.c_size_t()
    _check(_lib().bloomhip_compact(arr, ns, nr, on_dev, 1 if drop_tombstones else 0, optr,
                                   ctypes.byref(n_out), out_dev,
                                   filter.handle if filter is not None else None,
                                   filter.device if filter is not None else device,
                                   _stream_ptr(stream)), "bloomhip_compact")
    return out[:n_out.value]


# bloomhip_flush_batch's geometry (csrc/bloom_flush.h kFlushTile,
# kFlushBlockCap, kFlushScanChunk): the tiled radix sort ranks FLUSH_TILE ops
# per workgroup; a batch of at most FLUSH_BLOCK_CAP ops is sorted by one
# workgroup in one launch; the [digit][tile] counts are scanned in chunks of
# FLUSH_SCAN_CHUNK (FLUSH_SCAN_CHUNK // 256 tiles fill one chunk).
FLUSH_TILE = 4096
FLUSH_BLOCK_CAP = 8192
FLUSH_SCAN_CHUNK = 16384


def flush_batch(ops, drop_tombstones: bool = False, filter: BloomFilter | None = None,
                device: int = 0, out=None, stream=None):
    """Batched PUT (bloomhip_flush_batch): ops = entry_t records in arrival
    order (an int32 [n, 2] numpy array or device tensor; a delete is a record
    whose value is VAL_NONE).  Returns the run a flush of them writes: one entry
    per key, keys ascending, the last op's value (a [n_out, 2] int32 array, or
    the first n_out rows of `out` when given); builds `filter` (and its run
    metadata) from the run's keys when given."""
    dt = str(ops.dtype)
    if dt not in ("int32", "torch.int32") or len(ops.shape) != 2 or ops.shape[1] != 2:
        raise ValueError(f"ops must be an int32 [n, 2] entry_t array (got {dt} {tuple(ops.shape)})")
    ptr, on_dev, keep = _ptr_of(ops)
    n = _nbytes(keep) // 8
    if out is None:
        out = np.empty((max(n, 1), 2), dtype=np.int32)
    optr, out_dev, okeep = _out_ptr(out, n * 8, 4, "out")
    n_out = ctypes.c_size_t()
    _check(_lib().bloomhip_flush_batch(ptr if n else None, n, on_dev, 1 if drop_tombstones else 0,
                                       optr, ctypes.byref(n_out), out_dev,
                                       filter.handle if filter is not None else None,
                                       filter.device if filter is not None else device,
                                       _stream_ptr(stream)), "bloomhip_flush_batch")
    return out[:n_out.value]


# bloomhip_flush_cuts' walk (csrc/bloom_tree.h kTreeCutChunk): one workgroup
# takes the op stream in chunks of TREE_CUT_CHUNK ops, one per lane; chunk c is
# ops [c * TREE_CUT_CHUNK, (c + 1) * TREE_CUT_CHUNK).
TREE_CUT_CHUNK = 1024


def _ops_ptr(ops, what: str):
    dt = str(ops.dtype)
    if dt not in ("int32", "torch.int32") or len(ops.shape) != 2 or ops.shape[1] != 2:
        raise ValueError(f"{what} must be an int32 [n, 2] entry_t array (got {dt} {tuple(ops.shape)})")
    ptr, on_dev, keep = _ptr_of(ops)
    return ptr, on_dev, keep, _nbytes(keep) // 8


def flush_cuts(ops, buffer_max_entries: int, device: int = 0, cuts_cap: int | None = None,
               stream=None) -> np.ndarray:
    """Where the reference's buffer of `buffer_max_entries` flushes on `ops`
    (bloomhip_flush_cuts): ops = entry_t records in arrival order (an int32
    [n, 2] numpy array or device tensor).  Returns the realised cuts 0 < c_1 <
    ... < n as np.uint64: segment k is ops[c_{k-1}:c_k], the tail stays in the
    buffer.  cuts_cap (for tests) limits the output: BloomHipError(ERANGE) with
    the true count in its `ncuts` when there are more."""
    ptr, on_dev, keep, n = _ops_ptr(ops, "ops")
    B = int(buffer_max_entries)
    cap = (n // B + 1 if B > 0 else 0) if cuts_cap is None else int(cuts_cap)
    cuts = np.empty(max(cap, 1), dtype=np.uint64)
    nc = ctypes.c_size_t()
    rc = _lib().bloomhip_flush_cuts(ptr if n else None, n, on_dev, max(B, 0),
                                    cuts.ctypes.data if cap else None, cap, ctypes.byref(nc),
                                    device, _stream_ptr(stream))
    if rc != OK:
        err = BloomHipError(rc, "bloomhip_flush_cuts")
        err.ncuts = nc.value
        raise err
    return cuts[:nc.value].copy()


def tree_plan(runs_per_level, fanout: int, nflushes: int):
    """The plan LSMTree.put_batch builds its runs by (bloomhip_tree_plan_host;
    no GPU needed): from the runs per level before a batch and the number of
    flushes it makes, the final tree as a list of
    (level, first_new, n_new, [(old_level, old_index), ...]), level by level,
    newest first.  BloomHipError(ERANGE) when the reference would die with
    "No more space in tree"."""
    shape = np.ascontiguousarray(runs_per_level, dtype=np.uint32)
    depth = int(shape.size)
    ln = ctypes.c_size_t()
    L = _lib()
    rc = L.bloomhip_tree_plan_host(shape.ctypes.data, depth, int(fanout), int(nflushes), None, 0,
                                   ctypes.byref(ln))
    if rc != OK and not (rc == ERANGE and ln.value):
        raise BloomHipError(rc, "bloomhip_tree_plan_host")
    flat = np.empty(max(ln.value, 1), dtype=np.int32)
    _check(L.bloomhip_tree_plan_host(shape.ctypes.data, depth, int(fanout), int(nflushes),
                                     flat.ctypes.data, ln.value, ctypes.byref(ln)),
           "bloomhip_tree_plan_host")
    plan, o = [], 0
    while o < ln.value:
        level, first, n_new, n_old = (int(x) for x in flat[o:o + 4])
        olds = [(int(flat[o + 4 + 2 * j]), int(flat[o + 5 + 2 * j])) for j in range(n_old)]
        plan.append((level, first, n_new, olds))
        o += 4 + 2 * n_old
    return plan


class LSMTree:
    """The reference's LSMTree (src/lsm_tree.h:9-13 for the defaults) with
    batched ingest: a ``bloomhip_tree`` handle.  After any sequence of
    put_batch calls it holds exactly the tree the reference holds after the
    same ops put one by one."""

    def __init__(self, buffer_max_entries: int, depth: int = 5, fanout: int = 10,
                 bits_per_entry: float = 0.5, device: int = 0):
        h = ctypes.c_void_p()
        _check(_lib().bloomhip_tree_create(device, max(int(buffer_max_entries), 0), int(depth),
                                           int(fanout), float(bits_per_entry), ctypes.byref(h)),
               "bloomhip_tree_create")
        self._h = h
        self.buffer_max_entries = int(buffer_max_entries)
        self.depth, self.fanout = int(depth), int(fanout)
        self.bits_per_entry = float(bits_per_entry)
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib().bloomhip_tree_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def put_batch(self, ops, stream=None) -> int:
        """Puts and deletes in arrival order (int32 [n, 2] entry_t records, a
        delete carrying VAL_NONE; numpy array or device tensor).  Returns the
        number of flushes the reference makes on them.  BloomHipError(ERANGE)
        where it would die with "No more space in tree"; the tree is unchanged
        then."""
        ptr, on_dev, keep, n = _ops_ptr(ops, "ops")
        nf = ctypes.c_size_t()
        _check(_lib().bloomhip_tree_put_batch(self._h, ptr if n else None, n, on_dev,
                                              ctypes.byref(nf), _stream_ptr(stream)),
               "bloomhip_tree_put_batch")
        return nf.value

    def load(self, path: str) -> int:
        """LSMTree::load (src/lsm_tree.cpp:296-309): a put per entry_t record
        of a binary file."""
        raw = np.fromfile(path, dtype=np.int32)
        return self.put_batch(raw[:raw.size // 2 * 2].reshape(-1, 2))

    def get(self, keys, n: int | None = None, stride: int = 4, vals=None, found_run=None,
            stream=None):
        """Batched GET over the buffer and the runs.  Returns (vals int32[n],
        found_run int32[n]): VAL_NONE and -1 where no run holds the key (a
        tombstone's value is passed through); found_run is 0 for the buffer and
        1 + r for run r in get_run order.  Outputs are host arrays unless
        device tensors are given."""
        ptr, on_dev, keep = _keys_ptr(keys, stride)
        n = _key_count(keep, stride, n)
        if vals is None and found_run is None:
            vals = np.empty(n, dtype=np.int32)
            found_run = np.empty(n, dtype=np.int32)
        outs = [_out_ptr(x, n * 4, 4, w) if x is not None else (None, None, None)
                for x, w in ((vals, "vals"), (found_run, "found_run"))]
        devs = {o[1] for o in outs if o[0] is not None}
        if len(devs) > 1:
            raise ValueError("get outputs must be all host or all device buffers")
        _check(_lib().bloomhip_tree_get_batch(self._h, ptr, n, stride, on_dev, outs[0][0], outs[1][0],
                                              devs.pop() if devs else 0, _stream_ptr(stream)),
               "bloomhip_tree_get_batch")
        return vals, found_run

    def range(self, starts, ends, stream=None):
        """Batched RANGE: (offsets uint64[nq + 1], entries int32[total, 2]),
        query q's answer being entries[offsets[q]:offsets[q + 1]] (host arrays)."""
        sptr, s_dev, skeep = _keys_ptr(starts, 4)
        eptr, e_dev, ekeep = _keys_ptr(ends, 4)
        nq = _nbytes(skeep) // 4
        if _nbytes(ekeep) // 4 != nq:
            raise ValueError("starts and ends must have one length")
        if nq and s_dev != e_dev:
            raise ValueError("starts and ends must be both host or both device buffers")
        offsets = np.empty(nq + 1, dtype=np.uint64)
        total = ctypes.c_size_t()

        def call(buf, cap):
            return _lib().bloomhip_tree_range_batch(self._h, sptr, eptr, nq, s_dev, offsets.ctypes.data,
                                                    buf, cap, ctypes.byref(total), 0,
                                                    _stream_ptr(stream))

        _check(call(None, 0), "bloomhip_tree_range_batch")
        out = np.empty((total.value, 2), dtype=np.int32)
        if total.value:
            _check(call(out.ctypes.data, total.value), "bloomhip_tree_range_batch")
        return offsets, out

    def shape(self):
        """(runs per level, entries in the buffer)."""
        rpl = np.zeros(self.depth, dtype=np.uint32)
        mem = ctypes.c_uint64()
        _check(_lib().bloomhip_tree_shape(self._h, rpl.ctypes.data, ctypes.byref(mem)),
               "bloomhip_tree_shape")
        return [int(x) for x in rpl], mem.value

    def run(self, level: int, index: int = 0):
        """(entries int32[n, 2] on the host, BloomFilter view) of run `index`
        (0 = newest) of `level`; level -1 is the buffer as a key-sorted run.
        The view is the tree's own filter: valid until the next put_batch."""
        f, e, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        _check(_lib().bloomhip_tree_run(self._h, int(level), int(index), ctypes.byref(f),
                                        ctypes.byref(e), ctypes.byref(n)), "bloomhip_tree_run")
        view = BloomFilter._adopt(f, self.device)
        view._borrowed = True
        out = np.empty((n.value, 2), dtype=np.int32)
        if n.value:
            # a compaction of one run is a copy of it: device to host
            arr = (ctypes.c_void_p * 1)(e.value)
            ns = (ctypes.c_size_t * 1)(n.value)
            got = ctypes.c_size_t()
            _check(_lib().bloomhip_compact(arr, ns, 1, 1, 0, out.ctypes.data, ctypes.byref(got), 0,
                                           None, self.device, None), "bloomhip_compact")
            if got.value != n.value:
                raise BloomHipError(EIO, "LSMTree.run: the run's keys are not distinct")
        return out, view


# --- workload streams (generator/generator.c restatement) --------------------
def gen_mt19937(seed: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.uint32)
    _check(_lib().bloomhip_gen_mt19937(seed, n, out.ctypes.data), "gen_mt19937")
    return out


def gen_glibc_rand(seed: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.int32)
    _check(_lib().bloomhip_gen_glibc_rand(seed, n, out.ctypes.data), "gen_glibc_rand")
    return out


def gen_puts(seed: int, n: int, with_vals: bool = False):
    keys = np.empty(n, dtype=np.int32)
    vals = np.empty(n, dtype=np.int32) if with_vals else None
    _check(_lib().bloomhip_gen_puts(seed, n, keys.ctypes.data,
                                    vals.ctypes.data if with_vals else None), "gen_puts")
    return (keys, vals) if with_vals else keys


def gen_workload(seed: int, n_puts: int, n_gets: int, skew: float, miss_ratio: float):
    puts = np.empty(n_puts, dtype=np.int32)
    gets = np.empty(n_gets, dtype=np.int32)
    _check(_lib().bloomhip_gen_workload(seed, n_puts, n_gets, skew, miss_ratio,
                                        puts.ctypes.data, gets.ctypes.data), "gen_workload")
    return puts, gets
