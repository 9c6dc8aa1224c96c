// The route of a submit (scanner_amd/csrc/scn_host.hip: submit_route) as a stand-alone program: built by g++ -x c++ together with
// that unit, no HIP header on the include path, plain and under ASan + UBSan (tests/test_submit_route_cpp.py).  Every combination of
// the inputs on both sides of every threshold against what must hold of ANY route -- each stream that is made to wait is given an
// event, `done` is completed exactly once --, and a short table of routes written down from the measurement notes, not from the
// function's output.
#include <cstdio>

#include "scn_host.h"

static int g_failed = 0;
static SubmitShape g_in;
#define CHECK(cond)                                                                                                                \
  do {                                                                                                                             \
    if (!(cond)) {                                                                                                                 \
      std::printf("FAILED %s:%d: %s  (hits %d fused %d direct_counts %d own_stream %d list_wanted %d n %u units %u)\n", __FILE__,  \
                  __LINE__, #cond, g_in.hits, g_in.fused, g_in.direct_counts, g_in.own_stream, g_in.list_wanted, g_in.n, g_in.units); \
      g_failed++;                                                                                                                  \
    }                                                                                                                              \
  } while (0)

struct Expected {
  const char *what;
  SubmitShape in;
  Counts counts;
  RouteStream counts_stream;
  bool list_behind, list_forks;
  KernelEnd end;
  bool end_in_packet, done_behind_counts;
};

int main() {
  const uint32_t from = kTotalKernelFrom;
  const uint32_t shapes[][2] = {{16, 0},        {16, 1},      {16, 4096},   {16, 4097},   {16, from - 1u}, {16, from},
                                {128, from},    {4096, 8191}, {4096, 8192}, {8192, 4097}, {64, 1u << 19},  {16, 1u << 21}};
  uint32_t cells = 0;
  for (int hits = 0; hits < 2; hits++)
    for (int transform = 0; transform < 3; transform++)  // not fused; fused; fused with the plan's direct_counts
      for (int own = 0; own < 2; own++)
        for (int wanted = 0; wanted < 2; wanted++)
          for (const auto &sh : shapes) {
            const SubmitShape in = {hits != 0, transform >= 1, transform == 2, own != 0, wanted != 0, sh[0], sh[1]};
            g_in = in;
            const SubmitRoute r = submit_route(in);
            cells++;
            // with hits and units exactly one way for the counts, otherwise none
            CHECK((r.counts != Counts::None) == (in.hits && in.units != 0));
            CHECK(r.counts != Counts::Stored || in.fused);
            // (Counts is one value: the reduction and the kernel's stores cannot both be chosen; the reduction leaves the transform no pointer)
            CHECK(r.counts != Counts::Reduced || in.units >= from);
            // the list: behind the launch exactly for a submit with hits and units whose caller is known to want it
            CHECK(r.list_behind == (in.hits && in.units != 0 && in.list_wanted));
            CHECK(!r.list_forks || r.list_behind);
            // every stream other than the slot's that receives work waits on `end`: which the packet completes or a marker records
            const bool d2h_works = r.counts_stream == RouteStream::D2H;
            CHECK(!d2h_works || r.counts != Counts::None);  // (the D2H stream carries counts, never `done` alone)
            CHECK(!(d2h_works || r.list_forks) || r.end != KernelEnd::None);
            // `done` exactly once: as `end` (by the packet or the marker on the slot's stream) or behind the counts
            CHECK((r.end == KernelEnd::Done ? 1 : 0) + (r.done_behind_counts ? 1 : 0) == 1);
            // `kernel_done` only for a side stream to wait on; `done` as `end` only when nothing follows that the host waits for
            CHECK(r.end != KernelEnd::KernelDone || d2h_works || r.list_forks);
            CHECK(r.end != KernelEnd::Done || r.counts == Counts::None || r.counts == Counts::Stored);
            // completion by the packet: a fused transform, 2^25 samples, an event to complete
            CHECK(!r.end_in_packet || (in.fused && (uint64_t)in.n * in.units >= kPacketEventFrom && r.end != KernelEnd::None));
            // a slot with a stream of its own: nothing leaves it, no event but `done`
            if (in.own_stream) CHECK(r.counts_stream == RouteStream::Slot && !r.list_forks && r.end == KernelEnd::None && !r.end_in_packet);
          }
  CHECK(cells == 288u);

  // Routes as the notes in submit_route describe them.  Fused kernels store the counts themselves up to 4096 units, whenever the list
  // follows eagerly, and always from 8192 points (direct_counts); a DMA on the D2H stream carries them otherwise, behind `kernel_done`;
  // from 2^18 units the reduction on the slot's stream, with no event at all.  `done` is the kernel's end when nothing follows it on the
  // compute stream; the packet completes the event from 2^25 samples per launch.
  const bool F = false, T = true;
  const Expected table[] = {
      // the shapes of scripts/hip_call_sequence.py
      {"direct counts 4096 x 2048", {T, T, F, F, F, 4096, 2048}, Counts::Stored, RouteStream::Slot, F, F, KernelEnd::Done, F, F},
      {"eager list 4096 x 8192", {T, T, F, F, T, 4096, 8192}, Counts::Stored, RouteStream::Slot, T, T, KernelEnd::Done, T, F},
      {"total 16 x 262144", {T, T, F, F, F, 16, 262144}, Counts::Reduced, RouteStream::Slot, F, F, KernelEnd::None, F, T},
      {"average 2, 1024 x 8 (4 groups)", {T, F, F, F, F, 1024, 4}, Counts::Dma, RouteStream::D2H, F, F, KernelEnd::KernelDone, F, T},
      {"floor 64 x 8", {T, F, F, F, F, 64, 8}, Counts::Dma, RouteStream::D2H, F, F, KernelEnd::KernelDone, F, T},
      {"overlapped slots 4096 x 64, slot 0", {T, T, F, F, F, 4096, 64}, Counts::Stored, RouteStream::Slot, F, F, KernelEnd::Done, F, F},
      {"overlapped slots 4096 x 64, slot 1", {T, T, F, T, F, 4096, 64}, Counts::Stored, RouteStream::Slot, F, F, KernelEnd::None, F, T},
      {"floor 64 x 3000 with records", {T, F, F, F, T, 64, 3000}, Counts::Dma, RouteStream::D2H, T, T, KernelEnd::KernelDone, F, T},
      {"spectrum only 4096 x 8192", {F, T, F, F, F, 4096, 8192}, Counts::None, RouteStream::Slot, F, F, KernelEnd::Done, T, F},
      // an 8192-point plan: direct_counts, whatever the units
      {"8192 x 8192, direct_counts", {T, T, T, F, F, 8192, 8192}, Counts::Stored, RouteStream::Slot, F, F, KernelEnd::Done, T, F},
      // 4096 x 8192 without records: past 4096 units the counts go by DMA, and the packet completes `kernel_done`
      {"4096 x 8192, counts only", {T, T, F, F, F, 4096, 8192}, Counts::Dma, RouteStream::D2H, F, F, KernelEnd::KernelDone, T, T},
      // a transform that is not fused, eager, on the plan's stream, from 2^18 units: the list forks and needs an event, so no reduction
      {"floor 16 x 2^18 with records", {T, F, F, F, T, 16, 1u << 18}, Counts::Dma, RouteStream::D2H, T, T, KernelEnd::KernelDone, F, T},
      // ... and its neighbours keep the reduction: not eager; a stream of its own, where the list does not fork
      {"floor 16 x 2^18, counts only", {T, F, F, F, F, 16, 1u << 18}, Counts::Reduced, RouteStream::Slot, F, F, KernelEnd::None, F, T},
      {"floor 16 x 2^18 with records, own stream", {T, F, F, T, T, 16, 1u << 18}, Counts::Reduced, RouteStream::Slot, T, F, KernelEnd::None, F, T},
  };
  if (from == (1u << 18))  // (a variant library moves the threshold the table's rows are written for)
    for (const Expected &e : table) {
      g_in = e.in;
      const SubmitRoute r = submit_route(e.in);
      const bool same = r.counts == e.counts && r.counts_stream == e.counts_stream && r.list_behind == e.list_behind && r.list_forks == e.list_forks &&
                        r.end == e.end && r.end_in_packet == e.end_in_packet && r.done_behind_counts == e.done_behind_counts;
      if (!same) std::printf("route differs: %s\n", e.what);
      CHECK(same);
    }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("submit route tests ok (%u cells)\n", cells);
  return 0;
}
