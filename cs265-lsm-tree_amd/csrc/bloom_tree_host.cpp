// bloom_tree_host.cpp — the LSM tree handle (bloomhip_tree_*): batched ingest
// that ends in exactly the tree the reference would hold, and batched GET and
// RANGE over it.  Host code over the engine's own C ABI: bloomhip_flush_cuts
// finds where Buffer::put refuses, the plan below says which final run is made
// of which slice of the op stream and which old runs, bloomhip_flush_batch and
// bloomhip_compact build every final run once.
//
// Reference (jackdent/cs265-lsm-tree): LSMTree::LSMTree src/lsm_tree.cpp:28-42,
// merge_down :44-102, put :104-139, get_run :141-151, get :173-215,
// range :218-290; Buffer::put src/buffer.cpp:37-58; Run::Run src/run.cpp:13-15.
//
// Newest-wins is associative, so a run that merge_down produces out of runs
// that were themselves flushed or merged during this batch is the
// de-duplicated image of one contiguous slice of the op stream, merged with
// the old runs that went into it.  Tombstones are dropped only by a merge into
// the last level, and what that merge writes stays in the last level, so
// dropping them once, when the final run of the last level is built, leaves
// the same entries as dropping them merge by merge.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/bloomhip.h"

namespace {

constexpr int kTreeMaxRuns = 64;  // bloomhip_get_batch's and bloomhip_range_batch's limit

// A run of the plan: new segments [a, a + nnew), then old runs newest first.
struct PlanRun {
    uint64_t a = 0, nnew = 0;
    std::vector<std::pair<int, int>> olds;  // (level, index newest first) before the batch
};
using PlanLevels = std::vector<std::vector<PlanRun>>;  // [level][newest first]

// LSMTree::merge_down (src/lsm_tree.cpp:44-102) on shapes.  false: "No more
// space in tree".
bool plan_merge_down(PlanLevels &lv, int l, int fanout) {
    if ((int)lv[l].size() < fanout) return true;
    if (l + 1 >= (int)lv.size()) return false;
    if ((int)lv[l + 1].size() >= fanout && !plan_merge_down(lv, l + 1, fanout)) return false;
    PlanRun m;
    bool any_new = false;
    for (const PlanRun &r : lv[l]) {  // newest first
        if (r.nnew) {
            m.a = any_new ? std::min(m.a, r.a) : r.a;
            m.nnew += r.nnew;
            any_new = true;
        }
        m.olds.insert(m.olds.end(), r.olds.begin(), r.olds.end());
    }
    lv[l].clear();
    lv[l + 1].insert(lv[l + 1].begin(), std::move(m));
    return true;
}

// The tree after nflushes flushes of segments 0, 1, ...; false: no more space.
bool plan_tree(const uint32_t *runs_per_level, int depth, int fanout, uint64_t nflushes,
               PlanLevels *out) {
    PlanLevels lv(depth);
    for (int l = 0; l < depth; l++)
        for (uint32_t i = 0; i < runs_per_level[l]; i++) {
            PlanRun r;
            r.olds.push_back({l, (int)i});
            lv[l].push_back(std::move(r));
        }
    for (uint64_t k = 0; k < nflushes; k++) {
        if (!plan_merge_down(lv, 0, fanout)) return false;
        PlanRun r;
        r.a = k;
        r.nnew = 1;
        lv[0].insert(lv[0].begin(), std::move(r));
    }
    out->swap(lv);
    return true;
}

bool plan_kept(const PlanRun &r, int level) {
    return r.nnew == 0 && r.olds.size() == 1 && r.olds[0].first == level;
}

// The most flushes a tree of this geometry can take from empty:
// sum of fanout^(l+1); more always ends in "No more space".
uint64_t tree_flush_capacity(int depth, int fanout) {
    uint64_t cap = 0, p = 1;
    for (int l = 0; l < depth; l++) {
        if (p > (1ull << 40) / (uint64_t)fanout) return 1ull << 40;
        p *= (uint64_t)fanout;
        cap += p;
    }
    return cap;
}

struct TreeRun {
    bloomhip_filter *f = nullptr;
    void *d_entries = nullptr;
    size_t n = 0;
};

void free_run(TreeRun *r) {
    if (!r) return;
    if (r->f) (void)bloomhip_destroy(r->f);
    if (r->d_entries) (void)hipFree(r->d_entries);
    delete r;
}

struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess || prev == dev) prev = -1;
        (void)hipSetDevice(dev);
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace

struct bloomhip_tree {
    int device = 0;
    uint64_t B = 0;
    int depth = 0, fanout = 0;
    float bpe = 0.f;
    std::vector<uint64_t> m_level;  // filter bits of a run of level l
    uint64_t m_mem = 0;
    mutable std::mutex mu;
    std::vector<std::vector<TreeRun *>> levels;  // [level][newest first]
    TreeRun *mem = nullptr;                      // the buffer, as a sorted run
    void *d_stage = nullptr;                     // [memtable entries | ops] of a batch
    size_t stage_bytes = 0;
};

namespace {

int hip_rc(hipError_t e) {
    if (e == hipSuccess) return BLOOMHIP_OK;
    if (e == hipErrorOutOfMemory) return BLOOMHIP_ENOMEM;
    return BLOOMHIP_EIO;
}

// A new run with a filter of m bits and room for cap entries.
int new_run(int device, uint64_t m, size_t cap, TreeRun **out) {
    std::unique_ptr<TreeRun, void (*)(TreeRun *)> r(new TreeRun, free_run);
    int rc = bloomhip_create(device, m, &r->f);
    if (rc) return rc;
    rc = hip_rc(hipMalloc(&r->d_entries, std::max<size_t>(cap, 1) * 8));
    if (rc) return rc;
    *out = r.release();
    return BLOOMHIP_OK;
}

// The run list of a query: the memtable, then the runs in get_run order
// (src/lsm_tree.cpp:141-151).  Empty runs stay in the list with no entries
// when keep_empty (GET: found_run then numbers the runs as the shape does; a
// run of no keys has no fences and is never a candidate), else they are left
// out (RANGE), the memtable standing in when nothing else is there.
void query_runs(const bloomhip_tree *t, bool keep_empty, std::vector<const bloomhip_filter *> *fs,
                std::vector<const void *> *es, std::vector<size_t> *ns) {
    auto add = [&](const TreeRun *r) {
        fs->push_back(r->f);
        es->push_back(r->n ? r->d_entries : nullptr);
        ns->push_back(r->n);
    };
    if (keep_empty || t->mem->n) add(t->mem);
    for (const auto &lv : t->levels)
        for (const TreeRun *r : lv)
            if (keep_empty || r->n) add(r);
    if (fs->empty()) add(t->mem);
}

}  // namespace

extern "C" {

int bloomhip_tree_plan_host(const uint32_t *runs_per_level, int depth, int fanout,
                            uint64_t nflushes, int32_t *plan, size_t plan_cap,
                            size_t *plan_len_out) {
    if (!runs_per_level || depth < 1 || fanout < 1 || !plan_len_out || (plan_cap && !plan))
        return BLOOMHIP_EINVAL;
    if ((int64_t)depth * fanout > (1 << 20)) return BLOOMHIP_ERANGE;
    for (int l = 0; l < depth; l++)
        if (runs_per_level[l] > (uint32_t)fanout) return BLOOMHIP_EINVAL;
    *plan_len_out = 0;
    // segment numbers are int32 in the plan, and no tree takes more flushes
    // than its capacity
    if (nflushes > tree_flush_capacity(depth, fanout) || nflushes > 0x7FFFFFFFull)
        return BLOOMHIP_ERANGE;
    PlanLevels lv;
    if (!plan_tree(runs_per_level, depth, fanout, nflushes, &lv)) return BLOOMHIP_ERANGE;
    size_t len = 0;
    for (int l = 0; l < depth; l++)
        for (const PlanRun &r : lv[l]) len += 4 + 2 * r.olds.size();
    *plan_len_out = len;
    if (len > plan_cap) return BLOOMHIP_ERANGE;
    size_t o = 0;
    for (int l = 0; l < depth; l++)
        for (const PlanRun &r : lv[l]) {
            plan[o++] = l;
            plan[o++] = (int32_t)r.a;
            plan[o++] = (int32_t)r.nnew;
            plan[o++] = (int32_t)r.olds.size();
            for (const auto &od : r.olds) {
                plan[o++] = od.first;
                plan[o++] = od.second;
            }
        }
    return BLOOMHIP_OK;
}

int bloomhip_tree_create(int device, uint64_t buffer_max_entries, int depth, int fanout,
                         float bits_per_entry, bloomhip_tree **out) {
    if (!out || buffer_max_entries == 0 || depth < 1 || fanout < 1) return BLOOMHIP_EINVAL;
    if (buffer_max_entries > (uint64_t)INT64_MAX) return BLOOMHIP_ERANGE;
    uint64_t m0 = 0;
    if (bloomhip_m_bits((int64_t)buffer_max_entries, bits_per_entry, &m0) != BLOOMHIP_OK || m0 == 0)
        return BLOOMHIP_EINVAL;  // the reference divides by zero there
    if ((int64_t)depth * fanout + 1 > kTreeMaxRuns) return BLOOMHIP_ERANGE;
    std::vector<uint64_t> m_level;
    uint64_t cap = buffer_max_entries;  // B * fanout^l (src/lsm_tree.cpp:36-41)
    for (int l = 0; l < depth; l++) {
        uint64_t m = 0;
        if (bloomhip_m_bits((int64_t)cap, bits_per_entry, &m) != BLOOMHIP_OK || m == 0)
            return BLOOMHIP_ERANGE;
        m_level.push_back(m);
        if (l + 1 < depth) {
            if (cap > (uint64_t)INT64_MAX / (uint64_t)fanout) return BLOOMHIP_ERANGE;
            cap *= (uint64_t)fanout;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BLOOMHIP_ENODEV;
    if (device < 0 || device >= ndev) return BLOOMHIP_EINVAL;
    DeviceScope g(device);
    std::unique_ptr<bloomhip_tree> t(new bloomhip_tree);
    t->device = device;
    t->B = buffer_max_entries;
    t->depth = depth;
    t->fanout = fanout;
    t->bpe = bits_per_entry;
    t->m_level = std::move(m_level);
    t->m_mem = m0;
    t->levels.resize(depth);
    int rc = new_run(device, m0, 0, &t->mem);
    if (rc) return rc;
    *out = t.release();
    return BLOOMHIP_OK;
}

int bloomhip_tree_destroy(bloomhip_tree *t) {
    if (!t) return BLOOMHIP_OK;
    {
        std::lock_guard<std::mutex> lk(t->mu);
        DeviceScope g(t->device);
        for (auto &lv : t->levels)
            for (TreeRun *r : lv) free_run(r);
        free_run(t->mem);
        if (t->d_stage) (void)hipFree(t->d_stage);
    }
    delete t;
    return BLOOMHIP_OK;
}

int bloomhip_tree_put_batch(bloomhip_tree *t, const void *ops, size_t n, int ops_on_device,
                            size_t *nflushes_out, void *stream) {
    if (!t || (n && !ops)) return BLOOMHIP_EINVAL;
    if (n && (reinterpret_cast<uintptr_t>(ops) & (ops_on_device ? 7 : 3))) return BLOOMHIP_EINVAL;
    std::lock_guard<std::mutex> lk(t->mu);
    if (nflushes_out) *nflushes_out = 0;
    const uint64_t n_mem = t->mem->n;
    const uint64_t total = n_mem + n;
    if (total >= 0xFFFFFFFFull) return BLOOMHIP_ERANGE;
    if (n == 0) return BLOOMHIP_OK;
    DeviceScope g(t->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);

    // [memtable entries | ops]: the memtable's keys are distinct, so their
    // order does not matter, and a full memtable puts the first cut before ops[0]
    if (t->stage_bytes < total * 8) {
        if (t->d_stage) (void)hipFree(t->d_stage);
        t->d_stage = nullptr;
        t->stage_bytes = 0;
        const size_t want = std::max<size_t>(total * 8, 1 << 16);
        int rc = hip_rc(hipMalloc(&t->d_stage, want));
        if (rc) return rc;
        t->stage_bytes = want;
    }
    char *stage = static_cast<char *>(t->d_stage);
    if (n_mem) {
        int rc = hip_rc(hipMemcpyAsync(stage, t->mem->d_entries, n_mem * 8, hipMemcpyDeviceToDevice, s));
        if (rc) return rc;
    }
    {
        int rc = hip_rc(hipMemcpyAsync(stage + n_mem * 8, ops, n * 8,
                                       ops_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        if (rc) return rc;
        rc = hip_rc(hipStreamSynchronize(s));
        if (rc) return rc;
    }

    // where Buffer::put refuses
    std::vector<uint64_t> cuts((total - 1) / t->B + 1);
    size_t ncuts = 0;
    int rc = bloomhip_flush_cuts(stage, total, 1, t->B, cuts.data(), cuts.size(), &ncuts, t->device,
                                 stream);
    if (rc) return rc;
    cuts.resize(ncuts);

    // which final run is made of what
    std::vector<uint32_t> shape(t->depth);
    for (int l = 0; l < t->depth; l++) shape[l] = (uint32_t)t->levels[l].size();
    PlanLevels plan;
    if (ncuts > tree_flush_capacity(t->depth, t->fanout) ||
        !plan_tree(shape.data(), t->depth, t->fanout, ncuts, &plan))
        return BLOOMHIP_ERANGE;  // "No more space in tree"; nothing was changed

    // build everything new first, then swap
    std::vector<TreeRun *> fresh;  // owned here until the commit
    auto fail = [&](int code) {
        for (TreeRun *r : fresh) free_run(r);
        return code;
    };
    auto seg_begin = [&](uint64_t k) { return k == 0 ? 0 : cuts[k - 1]; };
    std::vector<std::vector<TreeRun *>> next(t->depth);
    std::vector<char> kept_flag;  // per old run, flattened
    std::vector<size_t> level_off(t->depth + 1, 0);
    for (int l = 0; l < t->depth; l++) level_off[l + 1] = level_off[l] + t->levels[l].size();
    kept_flag.assign(level_off[t->depth], 0);
    void *d_tmp = nullptr;  // the new part of a run that also has old runs
    struct TmpFree {
        void **p;
        ~TmpFree() {
            if (*p) (void)hipFree(*p);
        }
    } tmp_free{&d_tmp};
    for (int l = 0; l < t->depth; l++) {
        const bool last = l == t->depth - 1;
        for (const PlanRun &pr : plan[l]) {
            if (plan_kept(pr, l)) {
                const int idx = pr.olds[0].second;
                next[l].push_back(t->levels[l][idx]);
                kept_flag[level_off[l] + idx] = 1;
                continue;
            }
            const uint64_t lo = pr.nnew ? seg_begin(pr.a) : 0;
            const uint64_t hi = pr.nnew ? cuts[pr.a + pr.nnew - 1] : 0;
            uint64_t cap = hi - lo;
            for (const auto &od : pr.olds) cap += t->levels[od.first][od.second]->n;
            if (cap >= 0xFFFFFFFFull) return fail(BLOOMHIP_ERANGE);
            TreeRun *r = nullptr;
            rc = new_run(t->device, t->m_level[l], cap, &r);
            if (rc) return fail(rc);
            fresh.push_back(r);
            next[l].push_back(r);
            if (pr.olds.empty()) {
                // new segments only: a flush into level 0 keeps tombstones
                // (src/lsm_tree.cpp:124-129); deeper, the run went through a
                // merge, which drops them into the last level (:84-86)
                rc = bloomhip_flush_batch(stage + lo * 8, hi - lo, 1, last && l != 0, r->d_entries,
                                          &r->n, 1, r->f, t->device, stream);
                if (rc) return fail(rc);
                continue;
            }
            // the new part first, then the old runs newest first.  At most
            // depth * fanout old runs and one new part: within the 64 sources
            // of one merge (checked by bloomhip_tree_create).
            std::vector<const void *> src;
            std::vector<size_t> len;
            if (pr.nnew) {
                if (d_tmp) (void)hipFree(d_tmp);
                d_tmp = nullptr;
                rc = hip_rc(hipMalloc(&d_tmp, (hi - lo) * 8));
                if (rc) return fail(rc);
                size_t nn = 0;
                rc = bloomhip_flush_batch(stage + lo * 8, hi - lo, 1, 0, d_tmp, &nn, 1, nullptr,
                                          t->device, stream);
                if (rc) return fail(rc);
                src.push_back(d_tmp);
                len.push_back(nn);
            }
            for (const auto &od : pr.olds) {
                const TreeRun *o = t->levels[od.first][od.second];
                src.push_back(o->n ? o->d_entries : nullptr);
                len.push_back(o->n);
            }
            rc = bloomhip_compact(src.data(), len.data(), (int)src.size(), 1, last, r->d_entries,
                                  &r->n, 1, r->f, t->device, stream);
            if (rc) return fail(rc);
        }
    }
    // the tail becomes the new memtable: sorted, de-duplicated, tombstones kept
    const uint64_t tail = ncuts ? cuts[ncuts - 1] : 0;
    TreeRun *mem = nullptr;
    rc = new_run(t->device, t->m_mem, total - tail, &mem);
    if (rc) return fail(rc);
    fresh.push_back(mem);
    rc = bloomhip_flush_batch(stage + tail * 8, total - tail, 1, 0, mem->d_entries, &mem->n, 1, mem->f,
                              t->device, stream);
    if (rc) return fail(rc);

    // commit
    for (int l = 0; l < t->depth; l++)
        for (size_t i = 0; i < t->levels[l].size(); i++)
            if (!kept_flag[level_off[l] + i]) free_run(t->levels[l][i]);
    free_run(t->mem);
    t->levels.swap(next);
    t->mem = mem;
    if (nflushes_out) *nflushes_out = ncuts;
    return BLOOMHIP_OK;
}

int bloomhip_tree_get_batch(const bloomhip_tree *t, const void *keys, size_t n, size_t stride_bytes,
                            int keys_on_device, int32_t *vals, int32_t *found_run,
                            int out_on_device, void *stream) {
    if (!t) return BLOOMHIP_EINVAL;
    std::lock_guard<std::mutex> lk(t->mu);
    std::vector<const bloomhip_filter *> fs;
    std::vector<const void *> es;
    std::vector<size_t> ns;
    query_runs(t, true, &fs, &es, &ns);
    int rc = bloomhip_get_batch(fs.data(), es.data(), ns.data(), (int)fs.size(), 1, keys, n,
                                stride_bytes, keys_on_device, vals, found_run, nullptr,
                                out_on_device, stream);
    if (rc) return rc;
    // the run list is the tree's own: nothing of it may be in flight when the
    // lock is released
    return hip_rc(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
}

int bloomhip_tree_range_batch(const bloomhip_tree *t, const int32_t *starts, const int32_t *ends,
                              size_t nq, int bounds_on_device, uint64_t *offsets, void *out_entries,
                              size_t out_capacity, size_t *total_out, int out_on_device,
                              void *stream) {
    if (!t) return BLOOMHIP_EINVAL;
    std::lock_guard<std::mutex> lk(t->mu);
    std::vector<const bloomhip_filter *> fs;
    std::vector<const void *> es;
    std::vector<size_t> ns;
    query_runs(t, false, &fs, &es, &ns);
    return bloomhip_range_batch(fs.data(), es.data(), ns.data(), (int)fs.size(), 1, starts, ends, nq,
                                bounds_on_device, offsets, out_entries, out_capacity, total_out,
                                out_on_device, t->device, stream);
}

int bloomhip_tree_shape(const bloomhip_tree *t, uint32_t *runs_per_level,
                        uint64_t *memtable_entries) {
    if (!t) return BLOOMHIP_EINVAL;
    std::lock_guard<std::mutex> lk(t->mu);
    if (runs_per_level)
        for (int l = 0; l < t->depth; l++) runs_per_level[l] = (uint32_t)t->levels[l].size();
    if (memtable_entries) *memtable_entries = t->mem->n;
    return BLOOMHIP_OK;
}

int bloomhip_tree_run(const bloomhip_tree *t, int level, int index, const bloomhip_filter **f_out,
                      const void **entries_dev_out, size_t *nentries_out) {
    if (!t || level < -1 || level >= t->depth || index < 0) return BLOOMHIP_EINVAL;
    std::lock_guard<std::mutex> lk(t->mu);
    const TreeRun *r = nullptr;
    if (level == -1) {
        if (index != 0) return BLOOMHIP_EINVAL;
        r = t->mem;
    } else {
        if ((size_t)index >= t->levels[level].size()) return BLOOMHIP_EINVAL;
        r = t->levels[level][index];
    }
    if (f_out) *f_out = r->f;
    if (entries_dev_out) *entries_dev_out = r->d_entries;
    if (nentries_out) *nentries_out = r->n;
    return BLOOMHIP_OK;
}

}  // extern "C"
