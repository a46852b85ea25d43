// CPU driver of whisperkit_amd/csrc/devmem.h: the SAME owner and layout functions the library uses, built with g++ by tests/test_devmem.py
// (once more with -fsanitize=address,undefined).  One query per line on stdin, one answer line per query:
//   dec32 <d> <L> <V>   | mxabs <d> <L> | sxabs <d> <H> <B> | d32 <d> <B>
//        -> <measured size> <end of the carving pass> | region offsets of the measuring pass | region offsets of the carving pass
//   pack <what> <B> [<heads>]   what = nospeech | slots | forced | altf32 | inpassdev | inpassregion | rsdev | rshost | dtwdev | dtwhost | beamsum |
//                               aligntmp: a packed session buffer at B slots (aligntmp: <heads> alignment heads), with the library's own constants
//        -> <measured size> <end of the device pass> <end of the pinned pass> | region offsets measuring | against the device base | against the pinned base
//   ring <regions> <stride> <n> <n> ...   -> the element offset each take(n) of one StageRing returned, `full` where it refused
//   owner <k> <what>    -> a session-like sequence of allocations against a counting backend whose k-th allocation (what = alloc) or k-th
//                          zero-fill (what = fill) fails, k = 0: nothing fails; the sequence stops at the first error, the owner is destroyed:
//        -> <backend allocations tried> <error seen 0/1> <held before destruction> <live in the backend after> <freed twice or unknown>
//           <freed by the wrong kind> <library counter after - before> <pointers set that the owner did not hold>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "alternatives_plan.h"
#include "devmem.h"
#include "rule_sets_plan.h"

namespace {
// destinations with the field names and element widths of kernels.h Dec32LayerW / Dec32 / XabsLayerW / Xabs and of wh_model
using half = uint16_t;
struct pair32 { float x, y; };
struct Dec32Layer { const half *qkv_t, *o_t, *cq_t, *co_t, *fc1_t, *fc2_t; const float *qkv_g, *qkv_c, *cq_g, *cq_c, *fc1_g, *fc1_c; };
struct ModelTop { const half* emb_t; const float *lg_g, *lg_c; };
struct XabsLayer { const half *wkT, *wv_t; const float* bv; };
struct SessionXabs { half *qf_hi, *qf_lo; float* part; pair32* ml; };
struct SessionD32 { float *x, *q; half *za_hi, *za_lo, *zb_hi, *zb_lo, *h, *h_lo; pair32* stat; float* part; int* ticket; };

char* const kBase = reinterpret_cast<char*>(uintptr_t(0x7000) << 24);      // never dereferenced
std::vector<size_t> g_off;
template <class T> void note(const T* p, const void* base) { g_off.push_back((size_t)(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(base))); }

void note_dec32(const std::vector<Dec32Layer>& l, const ModelTop& m, const void* b) {
    for (const Dec32Layer& t : l) {
        note(t.qkv_t, b); note(t.o_t, b); note(t.cq_t, b); note(t.co_t, b); note(t.fc1_t, b); note(t.fc2_t, b);
        note(t.qkv_g, b); note(t.qkv_c, b); note(t.cq_g, b); note(t.cq_c, b); note(t.fc1_g, b); note(t.fc1_c, b);
    }
    note(m.emb_t, b); note(m.lg_g, b); note(m.lg_c, b);
}
void note_mxabs(const std::vector<XabsLayer>& l, const void* b) { for (const XabsLayer& t : l) { note(t.wkT, b); note(t.wv_t, b); } }
void note_sxabs(const SessionXabs& x, const void* b) { note(x.qf_hi, b); note(x.qf_lo, b); note(x.part, b); note(x.ml, b); }
void note_d32(const SessionD32& q, const void* b) {
    note(q.x, b); note(q.q, b); note(q.za_hi, b); note(q.za_lo, b); note(q.zb_hi, b); note(q.zb_lo, b); note(q.h, b); note(q.h_lo, b);
    note(q.stat, b); note(q.part, b); note(q.ticket, b);
}
void print_layout(size_t measured, size_t carved, size_t n_regions) {
    printf("%zu %zu |", measured, carved);
    for (size_t i = 0; i < g_off.size(); ++i) printf("%s %zu", i == n_regions ? " |" : "", g_off[i]);
    printf("\n");
    g_off.clear();
}

// ---- the packed session buffers.  The constants the library passes: kernels.h / common.h cannot be included here (HIP), the plan headers can
constexpr size_t kMaxTok = 224, kCtx = 1500, kDtwPathCap = 256 + 1500, kMaxSessionSlots = 256;
static_assert(wh::plan::kAltPositions == kMaxTok, "one alternatives row per decoder position");
char* const kBasePinned = reinterpret_cast<char*>(uintptr_t(0x5000) << 24);      // never dereferenced
template <class V, class Pack, class Note> void pack_query(Pack pack, Note note_view) {
    V v{};
    const size_t measured = pack(nullptr, v); note_view(v, nullptr);
    const size_t n_regions = g_off.size();
    const size_t dev = pack(kBase, v); note_view(v, kBase);
    const size_t pinned = pack(kBasePinned, v); note_view(v, kBasePinned);
    printf("%zu %zu %zu |", measured, dev, pinned);
    for (size_t i = 0; i < g_off.size(); ++i) printf("%s %zu", (i && i % n_regions == 0) ? " |" : "", g_off[i]);
    printf("\n");
    g_off.clear();
}
bool pack_dispatch(const char* what, size_t B, size_t H) {
    using namespace wh::mem;
    const std::string w = what;
    if (w == "nospeech") pack_query<NoSpeechView>([&](void* b, NoSpeechView& v) { return pack_nospeech(b, B, v); },
        [](const NoSpeechView& v, const void* b) { note(v.pos, b); note(v.stop, b); note(v.prob, b); note(v.stopped, b); note(v.cfg, b); });
    else if (w == "slots") pack_query<SlotTableView>([&](void* b, SlotTableView& v) { return pack_slot_table(b, B, v); },
        [](const SlotTableView& v, const void* b) { note(v.home, b); note(v.live, b); });
    else if (w == "forced") pack_query<ForcedOutView>([&](void* b, ForcedOutView& v) { return pack_forced_out(b, B, kMaxTok, v); },
        [](const ForcedOutView& v, const void* b) { note(v.lp, b); note(v.best, b); note(v.best_lp, b); });
    else if (w == "altf32") pack_query<AltF32View>([&](void* b, AltF32View& v) { return pack_alternatives_f32(b, B, wh::plan::kAltPositions, wh::plan::kMaxAlternatives, v); },
        [](const AltF32View& v, const void* b) { note(v.lp, b); note(v.entropy, b); });
    else if (w == "inpassdev") pack_query<InpassDevView>([&](void* b, InpassDevView& v) { return pack_inpass_dev(b, B, kMaxTok, v); },
        [](const InpassDevView& v, const void* b) { note(v.live, b); note(v.owner, b); });
    else if (w == "inpassregion") pack_query<InpassRegionView>([&](void* b, InpassRegionView& v) { return pack_inpass_region(b, B, kMaxTok, v); },
        [](const InpassRegionView& v, const void* b) { note(v.home, b); note(v.live, b); note(v.owner, b); });
    else if (w == "rsdev") pack_query<RuleSetsDevView>([&](void* b, RuleSetsDevView& v) { return pack_rule_sets_dev(b, wh::plan::kMaxRuleSets, kMaxSessionSlots, (size_t)wh::plan::kRuleSetBankWords, v); },
        [](const RuleSetsDevView& v, const void* b) { note(v.matches, b); note(v.slots, b); note(v.bank, b); });
    else if (w == "rshost") pack_query<RuleSetsHostView>([&](void* b, RuleSetsHostView& v) { return pack_rule_sets_host(b, kMaxSessionSlots, wh::plan::kRuleSetStride, v); },
        [](const RuleSetsHostView& v, const void* b) { note(v.slots, b); note(v.stage, b); });
    else if (w == "dtwdev" || w == "dtwhost") pack_query<DtwView>([&](void* b, DtwView& v) { return pack_dtw(b, B, kDtwPathCap, w == "dtwdev", v); },
        [](const DtwView& v, const void* b) { note(v.rows, b); note(v.len, b); note(v.ti, b); note(v.tj, b); });
    else if (w == "beamsum") pack_query<BeamSumView>([&](void* b, BeamSumView& v) { return pack_beam_sums(b, B, v); },
        [](const BeamSumView& v, const void* b) { note(v.half[0], b); note(v.half[1], b); });
    else if (w == "aligntmp") pack_query<AlignTmpView>([&](void* b, AlignTmpView& v) { return pack_align_tmp(b, kMaxTok, H, kCtx, v); },
        [](const AlignTmpView& v, const void* b) { note(v.rows, b); note(v.stat, b); note(v.flags, b); });
    else return false;
    return true;
}
void ring_query(const char* line) {
    size_t regions, stride; int used = 0;
    if (sscanf(line, "ring %zu %zu%n", &regions, &stride, &used) != 2) { printf("bad query\n"); return; }
    wh::mem::StageRing ring(regions, stride);
    size_t n; int more = 0;
    for (const char* p = line + used; sscanf(p, "%zu%n", &n, &more) == 1; p += more) {
        const size_t at = ring.take(n);
        if (at == wh::mem::StageRing::kFull) printf("full "); else printf("%zu ", at);
    }
    printf("| %zu\n", ring.taken());
}

// ---- the counting backend
struct Fake {
    using Err = int;
    static constexpr Err ok = 0, out_of_memory = 2;
    static std::map<void*, bool> live;        // pointer -> pinned
    static long allocs, fills, fail_alloc, fail_fill, bad_free, wrong_kind;
    static Err get(void** p, size_t n, bool pinned) {
        if (++allocs == fail_alloc) return out_of_memory;
        *p = malloc(1);
        live[*p] = pinned;
        return ok;
    }
    static Err put(void* p, bool pinned) {
        auto it = live.find(p);
        if (it == live.end()) { ++bad_free; return 1; }          // freed twice, or never handed out
        if (it->second != pinned) ++wrong_kind;
        live.erase(it);
        free(p);
        return ok;
    }
    static Err dev_malloc(void** p, size_t n) { return get(p, n, false); }
    static Err host_malloc(void** p, size_t n) { return get(p, n, true); }
    static Err dev_free(void* p) { return put(p, false); }
    static Err host_free(void* p) { return put(p, true); }
    static Err dev_memset(void* p, int, size_t) { return (live.count(p) && ++fills == fail_fill) ? 1 : ok; }
};
std::map<void*, bool> Fake::live;
long Fake::allocs, Fake::fills, Fake::fail_alloc, Fake::fail_fill, Fake::bad_free, Fake::wrong_kind;

// what a session does over its life: the creation-time buffers (zero-filled), one pinned mirror, then the lazy features - alignment rows
// re-sized once, their scratch re-sized once, the DTW pair, the beam buffers (one pinned), the slot table pair
struct Sequence {
    float* dev[64] = {};
    int* pinned[8] = {};
    int run(wh::mem::Owned<Fake>& o) {
#define TRY(e) do { if ((e) != Fake::ok) return 1; } while (0)
        int n = 0;
        for (; n < 40; ++n) TRY(o.alloc(&dev[n], 100 + n, true));
        TRY(o.alloc_pinned(&pinned[0], 16));
        TRY(o.alloc(&dev[n], 7, false));                                        // align
        o.release(dev[n]); dev[n] = nullptr; TRY(o.alloc(&dev[n], 9, false)); ++n;   // ... for another head set
        TRY(o.alloc(&dev[n], 5, false));                                        // align_tmp
        o.release(dev[n]); dev[n] = nullptr; TRY(o.alloc(&dev[n], 6, false)); ++n;
        o.release(nullptr);                                                      // nothing
        TRY(o.alloc(&dev[n++], 3, false)); TRY(o.alloc_pinned(&pinned[1], 3));   // DTW
        for (int i = 0; i < 11; ++i) TRY(o.alloc(&dev[n++], 50, false));         // beam
        TRY(o.alloc_pinned(&pinned[2], 4));
        TRY(o.alloc(&dev[n++], 2, false)); TRY(o.alloc_pinned(&pinned[3], 2));   // slot table
        return 0;
#undef TRY
    }
};

void owner_query(long k, bool fill) {
    Fake::live.clear();
    Fake::allocs = Fake::fills = Fake::bad_free = Fake::wrong_kind = 0;
    Fake::fail_alloc = fill ? 0 : k; Fake::fail_fill = fill ? k : 0;
    const long long before = wh::mem::g_live.load();
    int err; size_t held; long stray = 0;
    {
        wh::mem::Owned<Fake> o;
        Sequence q;
        err = q.run(o);
        held = o.held();
        // every pointer the sequence holds is one the backend knows (a failed allocation leaves its destination null) ...
        for (float* p : q.dev) if (p && !Fake::live.count(p)) ++stray;
        for (int* p : q.pinned) if (p && !Fake::live.count(p)) ++stray;
        if (held != Fake::live.size()) ++stray;          // ... and the owner holds exactly what is live
    }
    printf("%ld %d %zu %zu %ld %ld %lld %ld\n", Fake::allocs, err, held, Fake::live.size(), Fake::bad_free, Fake::wrong_kind, wh::mem::g_live.load() - before, stray);
}
}  // namespace

int main() {
    char line[4096];      // (a ring query lists every take)
    while (fgets(line, sizeof(line), stdin)) {
        size_t d, a, b;
        long k;
        char what[16];
        if (sscanf(line, "dec32 %zu %zu %zu", &d, &a, &b) == 3) {
            std::vector<Dec32Layer> l(a); ModelTop m{};
            const size_t measured = wh::mem::carve_model_dec32(nullptr, d, a, b, l.data(), m);
            note_dec32(l, m, nullptr);
            const size_t carved = wh::mem::carve_model_dec32(kBase, d, a, b, l.data(), m);
            note_dec32(l, m, kBase);
            print_layout(measured, carved, 12 * a + 3);
        } else if (sscanf(line, "mxabs %zu %zu", &d, &a) == 2) {
            std::vector<XabsLayer> l(a);
            const size_t measured = wh::mem::carve_model_xabs(nullptr, d, a, l.data());
            note_mxabs(l, nullptr);
            const size_t carved = wh::mem::carve_model_xabs(kBase, d, a, l.data());
            note_mxabs(l, kBase);
            print_layout(measured, carved, 2 * a);
        } else if (sscanf(line, "sxabs %zu %zu %zu", &d, &a, &b) == 3) {
            SessionXabs x{};
            const size_t measured = wh::mem::carve_session_xabs(nullptr, d, a, b, x);
            note_sxabs(x, nullptr);
            const size_t carved = wh::mem::carve_session_xabs(kBase, d, a, b, x);
            note_sxabs(x, kBase);
            print_layout(measured, carved, 4);
        } else if (sscanf(line, "d32 %zu %zu", &d, &a) == 2) {
            SessionD32 q{};
            const size_t measured = wh::mem::carve_session_d32(nullptr, d, a, q);
            note_d32(q, nullptr);
            const size_t carved = wh::mem::carve_session_d32(kBase, d, a, q);
            note_d32(q, kBase);
            print_layout(measured, carved, 11);
        } else if (sscanf(line, "pack %15s %zu %zu", what, &a, &b) >= 2) {
            if (!pack_dispatch(what, a, b)) printf("bad query\n");
        } else if (!strncmp(line, "ring ", 5)) {
            ring_query(line);
        } else if (sscanf(line, "owner %ld %15s", &k, what) == 2) {
            owner_query(k, !strcmp(what, "fill"));
        } else {
            printf("bad query\n");
        }
    }
    return 0;
}
