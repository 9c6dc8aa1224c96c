// What one SampleQueue::AppendSamples costs the producer on the zero-copy path, on the CPU alone (no GPU, no HIP): one producer thread
// appends 32 KiB short-complex buffers into a queue with one attached staging ring, then with two; a ring is 4 slots of 2048 buffers
// in ordinary memory, and its consumer thread takes a batch, marks it processed and releases the slot at once.  Prints ns per append.
// A tool for comparing two builds of the host sources (profiles/sample_queue_split.md), not a test:
//   g++ -std=gnu++11 -O2 -pthread -I scanner_amd/host scripts/ubench/append_rate.cpp scanner_amd/host/messageQueue.cpp
//       scanner_amd/host/captureWriter.cpp -o scripts/ubench/append_rate; scripts/ubench/append_rate [appends]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "messageQueue.h"

static double run(int nRings, size_t total) {
  const uint32_t n = 8192, depth = 8192, batch = 2048, nSlots = 4;  // 8192 x int16 IQ = 32 KiB
  SampleQueue q(SampleQueue::ShortComplex, 12, n, depth, false, false);
  std::vector<std::vector<unsigned char>> mem((size_t)nRings * nSlots, std::vector<unsigned char>((size_t)batch * n * 4));
  std::vector<int> ring(nRings);
  for (int r = 0; r < nRings; r++) {
    void *bases[nSlots];
    for (uint32_t s = 0; s < nSlots; s++) bases[s] = mem[(size_t)r * nSlots + s].data();
    ring[r] = q.AttachStaging(bases, nSlots, batch);
    if (ring[r] < 0) {
      fprintf(stderr, "AttachStaging refused\n");
      exit(1);
    }
  }
  std::vector<std::thread> consumers;
  for (int r = 0; r < nRings; r++)
    consumers.emplace_back([&q, &ring, r] {
      std::vector<SampleQueue::MessageType *> out;
      int slot = -1;
      while (q.TakeStagedBatch(ring[r], out, &slot, true, 40)) {
        for (SampleQueue::MessageType *m : out) q.MessageProcessed(m);
        out.clear();
        q.ReleaseStaging(ring[r], slot);
      }
    });
  std::vector<int16_t> src(64 * (size_t)n * 2, 3);  // 2 MiB of source, cycled: it stays in cache as a front-end's buffer does
  double ns = 0;
  std::thread producer([&] {
    q.AppendSamples(reinterpret_cast<int16_t(*)[2]>(src.data()), 0, 1);  // the discarded warm-up sweep
    q.AppendSamples(reinterpret_cast<int16_t(*)[2]>(src.data()), 0, 2);
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < total; k++) q.AppendSamples(reinterpret_cast<int16_t(*)[2]>(src.data() + (k % 64) * n * 2), 1e6 * k, 0);
    ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / total;
    q.SetIsDone();
  });
  producer.join();
  for (std::thread &c : consumers) c.join();
  if (q.GetStagedAppendCount() != total + 1 || q.GetCopiedAppendCount() != 0) {
    fprintf(stderr, "not every append was staged\n");
    exit(1);
  }
  for (int r = 0; r < nRings; r++) q.DetachStaging(ring[r]);
  printf("rings=%d: %.1f ns per append (%zu appends, producer blocked %.3f s)\n", nRings, ns, total, q.GetProducerWaitSeconds());
  return ns;
}

int main(int argc, char **argv) {
  const size_t total = argc > 1 ? (size_t)atoll(argv[1]) : 200000;
  run(1, total);
  run(2, total);
  return 0;
}
