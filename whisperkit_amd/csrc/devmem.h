// Who owns device and pinned memory, and how one allocation is carved into regions.  Plain C++17 (no HIP headers), like launch_plan.h:
// the library instantiates Owned with the HIP calls (internal.h HipMem), tests/native/devmem_check.cpp with a counting fake, and the layout
// functions below (carve_*: blobs of 256-byte aligned regions; pack_*: the packed tables of the session's opt-in features) and the staging
// ring run there under g++ with the SAME code the library cuts its buffers with (tests/test_devmem.py).
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

// ---------------------------------------------------------------------------------------------- packed allocations
// The sibling of Carve for the small tables of the session's opt-in features: regions back to back at their natural alignment, nothing
// rounded, because single copies span several regions (the no-speech tables go up in one copy, the DTW lengths and paths come down in
// one).  Same discipline: a pack_* function lists the regions ONCE, runs against a null base to measure and against the device and the
// pinned allocation to fill a typed view of each; the session keeps the views and nothing else cuts these buffers.
class Pack {
public:
    explicit Pack(void* base) : base_(reinterpret_cast<uintptr_t>(base)) {}
    template <class T> void take(T*& p, size_t n) {
        off_ = (off_ + alignof(T) - 1) / alignof(T) * alignof(T);
        p = reinterpret_cast<T*>(base_ + off_);
        off_ += n * sizeof(T);
    }
    size_t size() const { return off_; }
private:
    uintptr_t base_;
    size_t off_ = 0;
};

// The views.  The pack_* functions take the destination as a template parameter like the carve_* ones; these are what the library passes.
struct NoSpeechView { int32_t* pos; float *stop, *prob; int32_t *stopped, *cfg; };
struct SlotTableView { int32_t *home, *live; };
struct ForcedOutView { float* lp; int32_t* best; float* best_lp; };
struct AltF32View { float *lp, *entropy; };
struct InpassDevView { int32_t *live, *owner; };
struct InpassRegionView { int32_t *home, *live, *owner; };
struct RuleSetsDevView { unsigned long long* matches; int32_t *slots, *bank; };
struct RuleSetsHostView { int32_t *slots, *stage; };
struct DtwView { int32_t *rows, *len, *ti, *tj; };
struct BeamSumView { float* half[2]; };
struct AlignTmpView { float *rows, *stat; int32_t* flags; };
template <class Seq> struct PrefillSeqView { Seq *master, *fin; };
struct PrefillTabView { int32_t *ended, *home, *owner; };

// no-speech detection, by home slot: scoring position | stop threshold | probability | stopped flag | (token, lane divisor)
template <class V> size_t pack_nospeech(void* base, size_t B, V& v) {
    Pack c(base);
    c.take(v.pos, B); c.take(v.stop, B); c.take(v.prob, B); c.take(v.stopped, B); c.take(v.cfg, 2);
    return c.size();
}
// the pinned side of the compacted-pass slot table: home slot | live flag of every compact slot
template <class V> size_t pack_slot_table(void* base, size_t B, V& v) {
    Pack c(base);
    c.take(v.home, B); c.take(v.live, B);
    return c.size();
}
// forced pass, one entry per position of a call (at most B sequences of max_tok tokens): log p(target) | argmax | log p(argmax)
template <class V> size_t pack_forced_out(void* base, size_t B, size_t max_tok, V& v) {
    const size_t cap = B * (max_tok - 1);
    Pack c(base);
    c.take(v.lp, cap); c.take(v.best, cap); c.take(v.best_lp, cap);
    return c.size();
}
// token alternatives, the fp32 buffer: log-probabilities [B][positions][n_max] | entropies [B][positions] (the kernel indexes both from one base)
template <class V> size_t pack_alternatives_f32(void* base, size_t B, size_t positions, size_t n_max, V& v) {
    Pack c(base);
    c.take(v.lp, B * positions * n_max); c.take(v.entropy, B * positions);
    return c.size();
}
// in-pass compaction on the device: live flags [B] | row -> owner rows [B][max_tok]
template <class V> size_t pack_inpass_dev(void* base, size_t B, size_t max_tok, V& v) {
    Pack c(base);
    c.take(v.live, B); c.take(v.owner, B * max_tok);
    return c.size();
}
// ... and one region of its pinned staging (a StageRing of them): home slots [B] | live flags [B] | owner rows [B][max_tok]
template <class V> size_t pack_inpass_region(void* base, size_t B, size_t max_tok, V& v) {
    Pack c(base);
    c.take(v.home, B); c.take(v.live, B); c.take(v.owner, B * max_tok);
    return c.size();
}
// per-audio rule sets on the device: 64-bit match counters [n_sets] | set of every home slot [n_slots] | the banked sets [bank_words]
template <class V> size_t pack_rule_sets_dev(void* base, size_t n_sets, size_t n_slots, size_t bank_words, V& v) {
    Pack c(base);
    c.take(v.matches, n_sets); c.take(v.slots, n_slots); c.take(v.bank, bank_words);
    return c.size();
}
// ... and pinned: the slot table's mirror [n_slots] | the staging of one set [set_words]
template <class V> size_t pack_rule_sets_host(void* base, size_t n_slots, size_t set_words, V& v) {
    Pack c(base);
    c.take(v.slots, n_slots); c.take(v.stage, set_words);
    return c.size();
}
// batched DTW: token rows [B] (the device buffer only: with_rows) | path lengths [B] | text indices [B][cap] | time indices [B][cap]
template <class V> size_t pack_dtw(void* base, size_t B, size_t cap, bool with_rows, V& v) {
    Pack c(base);
    c.take(v.rows, with_rows ? B : 0); c.take(v.len, B); c.take(v.ti, B * cap); c.take(v.tj, B * cap);
    return c.size();
}
// device beam ranking: the cumulative log-probabilities of both halves of the ping-pong, [B] each
template <class V> size_t pack_beam_sums(void* base, size_t B, V& v) {
    Pack c(base);
    c.take(v.half[0], B); c.take(v.half[1], B);
    return c.size();
}
// alignment post-processing scratch of one slot: softmax rows [max_tok][heads][ctx] | statistics [2][heads][ctx] | 256 row flags
template <class V> size_t pack_align_tmp(void* base, size_t max_tok, size_t heads, size_t ctx, V& v) {
    Pack c(base);
    c.take(v.rows, max_tok * heads * ctx); c.take(v.stat, 2 * heads * ctx); c.take(v.flags, 256);
    return c.size();
}

// prompt prefill, the decode states: master states [B] | finished states [B]
template <class V> size_t pack_prefill_seq(void* base, size_t B, V& v) {
    Pack c(base);
    c.take(v.master, B); c.take(v.fin, B);
    return c.size();
}
// ... and its tables: ended flags [B] | home slot of every virtual slot [B] | row -> owner rows [B][max_tok]
template <class V> size_t pack_prefill_tab(void* base, size_t B, size_t max_tok, V& v) {
    Pack c(base);
    c.take(v.ended, B); c.take(v.home, B); c.take(v.owner, B * max_tok);
    return c.size();
}

// ---------------------------------------------------------------------------------------------- staging ring
// A pinned buffer of `regions` regions of `stride` elements whose region k is uploaded stream-ordered (to the same offset of a device twin,
// or to tables of its own): every launch of a pass takes the next regions, so the host never writes one the stream has not consumed.  One
// ring per pass, on the caller's stack; what a full ring means is the caller's business.
class StageRing {
public:
    static constexpr size_t kFull = ~(size_t)0;
    StageRing(size_t regions, size_t stride) : regions_(regions), stride_(stride) {}
    // the element offset of the next n regions, or kFull (nothing is taken then)
    size_t take(size_t n) {
        if (n > regions_ - next_) return kFull;
        const size_t off = next_ * stride_;
        next_ += n;
        return off;
    }
    size_t taken() const { return next_; }
    size_t stride() const { return stride_; }
private:
    size_t regions_, stride_, next_ = 0;
};

}  // namespace mem
}  // namespace wh
