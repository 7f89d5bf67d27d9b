"""The batched RANGE's surface, checked without a GPU: the prototype in
include/bloomhip.h, the exported symbol, the Python binding's signature, the
build's lists of kernel sources, and the class caps mirrored in Python."""
import ctypes
import inspect
import os
import re

import bloomhip as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs265-lsm-tree_amd", "csrc")

PROTOTYPE = """
int bloomhip_range_batch(const bloomhip_filter *const *runs, const void *const *entries,
                         const size_t *nentries, int nruns, int entries_on_device,
                         const int32_t *starts, const int32_t *ends, size_t nq, int bounds_on_device,
                         uint64_t *offsets, void *out_entries, size_t out_capacity,
                         size_t *total_out, int out_on_device, int device, void *stream);
"""


def _squash(text):
    return re.sub(r"\s+", " ", text).strip()


def _header():
    with open(os.path.join(ROOT, "include", "bloomhip.h")) as fh:
        return fh.read()


def test_header_declares_exactly_the_prototype():
    text = _header()
    decls = re.findall(r"^int bloomhip_range_batch\([^;]*;", text, re.M)
    assert len(decls) == 1
    assert _squash(decls[0]) == _squash(PROTOTYPE)


def test_abi_version_and_profiler_slots_unchanged():
    text = _header()
    assert re.search(r"^#define BLOOMHIP_ABI_VERSION 1$", text, re.M)
    assert re.search(r"^#define BLOOMHIP_PROF_SLOTS 13$", text, re.M)
    assert bh.PROF_SLOTS == 13


def test_symbol_exported_and_listed():
    L = ctypes.CDLL(bh.LIB_PATH)
    assert hasattr(L, "bloomhip_range_batch")
    assert "bloomhip_range_batch" in bh.EXPORTED_SYMBOLS


def test_python_signature():
    sig = inspect.signature(bh.range_batch)
    assert list(sig.parameters) == ["runs", "entries", "starts", "ends", "out", "offsets", "device",
                                    "stream"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"out": None, "offsets": None, "device": 0, "stream": None}


def _make_var(name):
    with open(os.path.join(CSRC, "Makefile")) as fh:
        text = fh.read().replace("\\\n", " ")
    m = re.search(rf"^{name}\s*:?=\s*(.*)$", text, re.M)
    assert m, name
    return m.group(1).split()


def test_range_unit_is_built_and_in_the_digest():
    assert "bloom_range" in _make_var("KERNEL_UNITS")
    srcs = _make_var("KERNEL_SRCS")
    hdrs = _make_var("HDRS")
    for name in ("bloom_range.hip", "bloom_range.h", "bloom_search.h"):
        assert os.path.exists(os.path.join(CSRC, name))
        assert name in srcs, name
    assert "bloom_range.h" in hdrs and "bloom_search.h" in hdrs


def test_python_caps_equal_the_headers():
    with open(os.path.join(CSRC, "bloom_range.h")) as fh:
        text = fh.read()
    wave = int(re.search(r"constexpr uint32_t kRangeWaveCap = (\d+);", text).group(1))
    block = int(re.search(r"constexpr uint32_t kRangeBlockCap = (\d+);", text).group(1))
    per_lane = int(re.search(r"constexpr int kRangePerLane = (\d+);", text).group(1))
    assert (bh.RANGE_WAVE_CAP, bh.RANGE_BLOCK_CAP) == (wave, block)
    assert (wave, block) == (64 * per_lane, 256 * per_lane)
