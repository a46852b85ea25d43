// Who owns device and pinned memory, and how one allocation is carved into regions.  Plain C++17 (no HIP headers), like launch_plan.h:
// the library instantiates Owned with the HIP calls (internal.h HipMem), tests/native/devmem_check.cpp with a counting fake, and the four
// layout functions below run there under g++ with the SAME code the library carves with (tests/test_devmem.py).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "launch_plan.h"

namespace wh {
namespace mem {

// device + pinned allocations the owners of this process hold (wh_debug_live_allocations): touched at allocation and free only
inline std::atomic<long long> g_live{0};

// Hands out device and pinned allocations, remembers each one and frees them all in its destructor.  A model and a session hold one each
// (nothing else in the library frees their memory); a stand-alone entry point holds one on its stack for its temporaries.
// Backend: struct of static functions over `Err` (ok, out_of_memory): dev_malloc, dev_free, host_malloc, host_free, dev_memset.
// Not thread safe: the caller serialises, as it does for the object that holds the owner.
template <class Backend>
class Owned {
public:
    using Err = typename Backend::Err;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { for (const Rec& r : recs_) drop(r); }

    // n elements on the device; zero = filled by the backend's blocking memset.  On an error *p is what it was (the allocation failed) or
    // owned like any other (the fill failed).
    template <class T> Err alloc(T** p, size_t n, bool zero) { return get(p, n, false, zero); }
    template <class T> Err alloc_pinned(T** p, size_t n) { return get(p, n, true, false); }
    // free one allocation early (a buffer that is re-sized while its holder lives); null or not handed out by this owner: nothing happens
    void release(void* p) {
        for (size_t i = 0; p && i < recs_.size(); ++i)
            if (recs_[i].p == p) { drop(recs_[i]); recs_.erase(recs_.begin() + (long)i); return; }
    }
    size_t held() const { return recs_.size(); }

private:
    struct Rec { void* p; bool pinned; };
    std::vector<Rec> recs_;

    static void drop(const Rec& r) {
        if (r.pinned) Backend::host_free(r.p); else Backend::dev_free(r.p);
        g_live.fetch_sub(1, std::memory_order_relaxed);
    }
    template <class T> Err get(T** p, size_t n, bool pinned, bool zero) {
        try { recs_.reserve(recs_.size() + 1); } catch (const std::bad_alloc&) { return Backend::out_of_memory; }     // (before anything exists)
        void* v = nullptr;
        const Err e = pinned ? Backend::host_malloc(&v, n * sizeof(T)) : Backend::dev_malloc(&v, n * sizeof(T));
        if (e != Backend::ok) return e;
        if (!v) return Backend::ok;          // (an empty request)
        recs_.push_back(Rec{v, pinned});
        g_live.fetch_add(1, std::memory_order_relaxed);
        *p = static_cast<T*>(v);
        return zero ? Backend::dev_memset(v, 0, n * sizeof(T)) : Backend::ok;
    }
};

// ---------------------------------------------------------------------------------------------- carved allocations
// One allocation, many regions, each starting on a 256-byte boundary.  A layout function below lists the regions of one blob ONCE and runs
// twice: against a null base it measures (the return value is the allocation's size; the pointers it stores are the bare offsets, so the
// library measures into a scratch destination), against the allocation it hands out the pointers.  The size cannot disagree with the carving.
class Carve {
public:
    explicit Carve(void* base) : base_(reinterpret_cast<uintptr_t>(base)) {}
    template <class T> void take(T*& p, size_t n) {         // the element type is the destination's
        p = reinterpret_cast<T*>(base_ + off_);
        off_ = (off_ + n * sizeof(T) + 255) / 256 * 256;
    }
    size_t size() const { return off_; }
private:
    uintptr_t base_;
    size_t off_ = 0;
};

// The destinations are template parameters so that this header needs no device types: the library passes kernels.h Dec32LayerW / Dec32 /
// XabsLayerW / Xabs and wh_model, the CPU test structs with the same field names and element widths.

// model: the decoder's projection weights in MFMA tile order with their LayerNorm folds (decoder32.hip), then the tied embedding's
template <class Layer, class Model>
size_t carve_model_dec32(void* base, size_t d, size_t L, size_t V, Layer* layers, Model& m) {
    const size_t Vp = (V + 31) / 32 * 32;
    Carve c(base);
    for (size_t l = 0; l < L; ++l) {
        Layer& t = layers[l];
        c.take(t.qkv_t, 3 * d * d); c.take(t.o_t, d * d); c.take(t.cq_t, d * d); c.take(t.co_t, d * d); c.take(t.fc1_t, 4 * d * d); c.take(t.fc2_t, 4 * d * d);
        c.take(t.qkv_g, 3 * d); c.take(t.qkv_c, 3 * d); c.take(t.cq_g, d); c.take(t.cq_c, d); c.take(t.fc1_g, 4 * d); c.take(t.fc1_c, 4 * d);
    }
    c.take(m.emb_t, Vp * d); c.take(m.lg_g, Vp); c.take(m.lg_c, Vp);
    return c.size();
}

// model: the absorbed cross-attention's W_k^T and W_v tiles per layer (xabs.hip)
template <class Layer>
size_t carve_model_xabs(void* base, size_t d, size_t L, Layer* layers) {
    Carve c(base);
    for (size_t l = 0; l < L; ++l) { c.take(layers[l].wkT, d * d); c.take(layers[l].wv_t, d * d); }
    return c.size();
}

// session: absorbed queries (heads padded to 16 / 32) and the partial outputs + softmax statistics of every key split
template <class X>
size_t carve_session_xabs(void* base, size_t d, size_t H, size_t B, X& x) {
    const size_t nht = H > 16 ? 2 : 1, S = kXabsSplits;
    Carve c(base);
    c.take(x.qf_hi, B * nht * (d / 32) * 512); c.take(x.qf_lo, B * nht * (d / 32) * 512);
    c.take(x.part, S * H * (d / 8) * B * 8);
    c.take(x.ml, S * H * B);
    return c.size();
}

// session: decode-step activations of ceil(B / 32) batch tiles - residual, query, the hi | lo planes, statistics, split-K scratch + counters
template <class Q>
size_t carve_session_d32(void* base, size_t d, size_t B, Q& q) {
    const size_t n_bt = (B + 31) / 32, R = n_bt * 32;
    Carve c(base);
    c.take(q.x, R * d); c.take(q.q, R * d);
    c.take(q.za_hi, R * d); c.take(q.za_lo, R * d); c.take(q.zb_hi, R * d); c.take(q.zb_lo, R * d);
    c.take(q.h, R * 4 * d); c.take(q.h_lo, R * 4 * d);
    c.take(q.stat, n_bt * (d / 32) * 32);
    c.take(q.part, n_bt * (size_t)kD32PartFloats);
    c.take(q.ticket, n_bt * 4096);
    return c.size();
}

}  // namespace mem
}  // namespace wh
