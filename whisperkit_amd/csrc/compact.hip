// In-pass compaction (wh_session_set_inpass_compaction, launch_plan.h inpass_compact_plan / inpass_compose): the per-slot decode state of a pass that
// narrows between two step graphs moves on the device, stream-ordered behind the graph in flight - no host round trip.  Everything the step kernels keep
// per slot between steps is the slot's SeqState (token history, position, filter rules of the next sampling step, random lane, temperature): the residual
// stream, the planes, the statistics and the logits are rewritten by every step, the tickets are zero between launches.  So a switch is two copies of
// whole SeqStates through a home-indexed array:
//   park    seq_home[home[i]] = seq[i]                 for every compact slot i of the OLD layout that carries a window (active),
//   gather  seq[i] = seq_home[home[i]]                 for i < the NEW width with live[i] != 0; padding entries become inactive.
// Two launches: the phases read and write the same arrays in opposite directions and must not alias inside one grid.  rng_lane travels inside the state
// and stays the home slot.  One workgroup per slot, one 32-bit word per thread and round.
#include "kernels.h"

namespace wh {

constexpr int kSeqWords = (int)(sizeof(SeqState) / 4);
static_assert(sizeof(SeqState) % 4 == 0, "SeqState moves as 32-bit words");

// home == null: the pass was never compacted, slot i is home slot i
__global__ __launch_bounds__(256) void seq_park_kernel(const SeqState* __restrict__ seq, SeqState* __restrict__ seq_home, const int* __restrict__ home,
                                                       int width, int n_slots) {
    const int i = blockIdx.x;
    if (i >= width) return;
    if (!seq[i].active) return;                         // padding entries and slots outside the pass's mask: their home entry is not theirs
    const int h = home ? home[i] : i;
    if (h < 0 || h >= n_slots) return;
    const int* src = reinterpret_cast<const int*>(seq + i);
    int* dst = reinterpret_cast<int*>(seq_home + h);
    for (int k = threadIdx.x; k < kSeqWords; k += 256) dst[k] = src[k];
}

__global__ __launch_bounds__(256) void seq_gather_kernel(const SeqState* __restrict__ seq_home, SeqState* __restrict__ seq, const int* __restrict__ home,
                                                         const int* __restrict__ live, int width, int n_slots) {
    const int i = blockIdx.x;
    if (i >= width) return;
    int* dst = reinterpret_cast<int*>(seq + i);
    const int h = home[i];
    if (!live[i] || h < 0 || h >= n_slots) {            // padding: an inactive slot whose every field is in range
        for (int k = threadIdx.x; k < kSeqWords; k += 256) dst[k] = 0;
        return;
    }
    const int* src = reinterpret_cast<const int*>(seq_home + h);
    for (int k = threadIdx.x; k < kSeqWords; k += 256) dst[k] = src[k];
}

void launch_seq_park(const SeqState* seq, SeqState* seq_home, const int* home, int width, int n_slots, hipStream_t st) {
    if (width < 1) return;
    seq_park_kernel<<<width, 256, 0, st>>>(seq, seq_home, home, width, n_slots);
}
void launch_seq_gather(const SeqState* seq_home, SeqState* seq, const int* home, const int* live, int width, int n_slots, hipStream_t st) {
    if (width < 1) return;
    seq_gather_kernel<<<width, 256, 0, st>>>(seq_home, seq, home, live, width, n_slots);
}

}  // namespace wh
