// Every WH_* environment variable the library reads: one table, one getenv.  Plain C++ (no HIP headers): tests/native/launch_plan_check.cpp
// takes the defaults from the same table.  What a knob decides, and the measurements behind its default, stand beside the decision it
// feeds (launch_plan.h for the kernel choices, the call site for the rest); this file says only how each one is parsed and when.
//
// A row: X(name, parse, lo, hi, default, read, meaning)
//   FLAG     1 when the value starts with '1', else 0
//   DIGIT    the first character when it is a digit lo .. hi, else the default
//   INT      atoi of the value (the default when unset); outside lo .. hi -> the default
//   INT_UP8  INT, then rounded up to a multiple of 8
//   STR      the string itself (null when unset), through knob::text
//   ONCE     read at the first use in the process and kept (knob::once)
//   CALL     read at every call of the function that uses it (knob::now / knob::text): a process may change it between sessions
#pragma once
#include <climits>
#include <cstdlib>

#define WH_KNOB_TABLE(X) \
    X(WH_NO_GRAPH,          FLAG,    0, 1,       0,  ONCE, "decode loop without captured step graphs") \
    X(WH_GRAPH_CAP,         INT,     1, INT_MAX, 112, ONCE, "step graphs a session keeps before the oldest configuration goes (4 x 28)") \
    X(WH_DBG_HOST,          FLAG,    0, 1,       0,  ONCE, "one line per decode: host time inside graph launches against waiting for the device") \
    X(WH_NO_FUSED_SAMPLER,  FLAG,    0, 1,       0,  CALL, "greedy decodes take the separate sampler kernel instead of the logits epilogue") \
    X(WH_DBG,               FLAG,    0, 1,       0,  ONCE, "allocate the timeline probe buffer: the projection and absorbed-attention kernels stamp wall clocks") \
    X(WH_XATT_PASSES,       INT,     INT_MIN, INT_MAX, 0, ONCE, "cross-attention passes per workgroup, snapped to 2 / 4 / 6 / 8; 0 = from the head count") \
    X(WH_XATT_NOFENCE,      INT,     INT_MIN, INT_MAX, 1, ONCE, "0 restores the acquire fence of the cross-attention split combine") \
    X(WH_XATT_GATE_LEAD,    INT,     INT_MIN, INT_MAX, 0, ONCE, "workgroups before the end of a cross-attention launch at which the gate goes back") \
    X(WH_XATT_LDS,          INT,     INT_MIN, INT_MAX, 0, ONCE, "extra dynamic LDS bytes per cross-attention workgroup (caps the residency)") \
    X(WH_XATT_NT,           INT,     INT_MIN, INT_MAX, 1, ONCE, "0: cacheable instead of non-temporal cross K / V loads") \
    X(WH_XATT_GATE,         INT,     INT_MIN, INT_MAX, -1, ONCE, "cross-attention gate: 0 never, 1 always, -1 while the model carries more than one session") \
    X(WH_LN_V4,             INT,     INT_MIN, INT_MAX, 2, ONCE, "encoder LayerNorm: 2 vector kernel with non-temporal accesses, 1 plain vector kernel, 0 scalar kernel") \
    X(WH_ENC_ATTN_V1,       FLAG,    0, 1,       0,  ONCE, "encoder attention with the first kernel generation") \
    X(WH_XABS,              INT,     INT_MIN, INT_MAX, -1, CALL, "automatic cross-attention choice of a new session: 0 K / V rows, 1 absorbed, -1 by slot count") \
    X(WH_XABS_SPW,          INT,     1, 16,      0,  CALL, "slots per absorbed-attention workgroup of a new session (1 .. kXabsMaxSlotsPerWorkgroup); 0 = the caller's") \
    X(WH_XABS_MIN_SLOTS,    INT,     1, INT_MAX, 28, CALL, "slots from which a new session picks the absorbed form on its own (kXabsAutoMinSlots)") \
    X(WH_XABS_SPLITS,       INT,     1, 4,       0,  CALL, "key splits per slot of a new absorbed session (1 .. kXabsSplits); 0 = automatic") \
    X(WH_XABS_NT,           INT,     INT_MIN, INT_MAX, 1, ONCE, "0: cacheable instead of non-temporal loads of the encoder-output stream") \
    X(WH_XABS_ABLATE,       INT,     INT_MIN, INT_MAX, 0, ONCE, "timing probe with garbage results: 1 no LDS-DMA in the loop, 2 no S / softmax / P V work, 3 both") \
    X(WH_NO_GEMM256,        FLAG,    0, 1,       0,  ONCE, "encoder GEMMs never take the 256 x 256 tile kernels") \
    X(WH_GEMM_EPI_MODE,     DIGIT,   0, 2,       1,  ONCE, "256-tile epilogue: 0 direct, 1 staged through LDS, 2 direct with the bias fetched in one batch") \
    X(WH_GEMM_PERSIST,      INT,     INT_MIN, INT_MAX, 0, ONCE, "non-zero: the persistent 256-tile loop (Float16 operand form only)") \
    X(WH_GEMM_PERSIST_WGS,  INT_UP8, 1, INT_MAX, 0,  ONCE, "workgroups of the persistent grid; 0 = the CUs") \
    X(WH_GEMM_STAGGER,      INT,     INT_MIN, INT_MAX, 0, ONCE, "persistent loop: first-round start stagger handed to the kernel") \
    X(WH_GEMM_GM,           INT,     1, 64,      8,  ONCE, "persistent loop: row tiles per column group of the tile order") \
    X(WH_CU_PARTS,          INT,     INT_MIN, INT_MAX, 0, CALL, "sessions take turns at this many compute-unit partitions (>= 2)") \
    X(WH_CU_PART_EXTRA,     INT,     INT_MIN, INT_MAX, 0, CALL, "CUs by which neighbouring partitions overlap") \
    X(WH_STREAM_PRIORITIES, STR,     0, 0,       0,  CALL, "\"p0,p1,...\": queue priority of session k's stream = p[k % n]") \
    X(WH_COMM_TIMEOUT_S,    INT,     1, INT_MAX, 120, ONCE, "socket deadline of the TCP transport in seconds") \
    X(WH_COMM_TOKEN,        STR,     0, 0,       0,  CALL, "job token appended to a TCP unique id that carries none") \
    X(WH_D32_KS_RESID,      INT,     INT_MIN, INT_MAX, 0, ONCE, "K splits of the out projections; 0 = from WH_D32_TILE_KB") \
    X(WH_D32_KS_FC2,        INT,     INT_MIN, INT_MAX, 0, ONCE, "K splits of fc2; 0 = from WH_D32_TILE_KB") \
    X(WH_D32_KS_Q,          INT,     INT_MIN, INT_MAX, 0, ONCE, "K splits of the cross-query projection; 0 = from WH_D32_TILE_KB") \
    X(WH_D32_KS_WIDE,       INT,     INT_MIN, INT_MAX, 1, ONCE, "K splits of qkv, fc1 and the logits") \
    X(WH_D32_TILE_KB,       INT,     INT_MIN, INT_MAX, 96, ONCE, "largest weight slab of one projection workgroup in KB") \
    X(WH_D32_TC,            INT,     INT_MIN, INT_MAX, 0, ONCE, "cap on the k-tiles per chunk of the weight stream; 0 = from the batch-tile count") \
    X(WH_D32_TC_BT,         INT,     INT_MIN, INT_MAX, 5, ONCE, "first batch-tile count with small chunks") \
    X(WH_D32_RT2_TC,        INT,     INT_MIN, INT_MAX, 4, ONCE, "cap on the k-tiles per chunk with two row tiles per workgroup") \
    X(WH_D32_NTW,           INT,     INT_MIN, INT_MAX, -1, ONCE, "non-temporal weight loads: 0 never, 1 always, -1 for a single batch tile only") \
    X(WH_D32_RT_BT,         INT,     INT_MIN, INT_MAX, 4, ONCE, "first batch-tile count with two row tiles per workgroup (99 = never)") \
    X(WH_D32_RT4_BT,        INT,     INT_MIN, INT_MAX, 5, ONCE, "first batch-tile count with four row tiles per workgroup (99 = never)") \
    X(WH_D32_RT4_MODES,     INT,     INT_MIN, INT_MAX, 7, ONCE, "projections that may take four row tiles: bit 0 qkv, 1 fc1, 2 fc2")

namespace wh {
namespace knob {

enum Parse { FLAG, DIGIT, INT, INT_UP8, STR };
enum Read { ONCE, CALL };
struct Row { const char* name; Parse parse; int lo, hi, dflt; Read read; const char* meaning; };

#define WH_KNOB_ID(name, ...) name,
enum Id { WH_KNOB_TABLE(WH_KNOB_ID) kCount };
#undef WH_KNOB_ID
#define WH_KNOB_ROW(name, parse, lo, hi, dflt, read, meaning) {#name, parse, lo, hi, dflt, read, meaning},
constexpr Row kTable[] = {WH_KNOB_TABLE(WH_KNOB_ROW)};
#undef WH_KNOB_ROW

inline const char* text_of(Id k) { return getenv(kTable[k].name); }      // the library's only look at the environment
inline int value_of(Id k) {
    const Row& r = kTable[k];
    const char* e = text_of(k);
    if (r.parse == FLAG) return e && e[0] == '1';
    if (r.parse == DIGIT) return e && e[0] >= '0' + r.lo && e[0] <= '0' + r.hi ? e[0] - '0' : r.dflt;
    int v = e ? atoi(e) : r.dflt;
    if (v < r.lo || v > r.hi) v = r.dflt;
    return r.parse == INT_UP8 ? (v + 7) / 8 * 8 : v;
}

// The two accessors.  The table's read column is binding: a knob is reachable through the accessor of its row only.
template <Id K> int once() {
    static_assert(kTable[K].read == ONCE && kTable[K].parse != STR, "knobs.h: this knob is read at the call");
    static const int v = value_of(K);
    return v;
}
template <Id K> int now() {
    static_assert(kTable[K].read == CALL && kTable[K].parse != STR, "knobs.h: this knob is read once per process");
    return value_of(K);
}
template <Id K> const char* text() {      // now() of the two string knobs
    static_assert(kTable[K].read == CALL && kTable[K].parse == STR, "knobs.h: not a string knob");
    return text_of(K);
}

}  // namespace knob
}  // namespace wh
