#include "messageQueue.h"

#include <cassert>
#include <chrono>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

// Copy into a pinned submit slot.  The destination is read next by the GPU's DMA engine, never by this core, so the
// stores bypass the cache (no read-for-ownership of lines that are about to be overwritten whole, and the source
// stays cached): on one core of the test host a 32 KiB buffer takes 1.6 us this way against 3.0 us with memcpy.
static void stream_copy(unsigned char *dst, const unsigned char *src, size_t bytes) {
#if defined(__SSE2__)
  if (((uintptr_t)dst & 15u) == 0 && bytes >= 256) {
    const size_t blocks = bytes / 64;
    for (size_t i = 0; i < blocks; i++) {
      const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src) + 4 * i);
      const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src) + 4 * i + 1);
      const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src) + 4 * i + 2);
      const __m128i d = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src) + 4 * i + 3);
      _mm_stream_si128(reinterpret_cast<__m128i *>(dst) + 4 * i, a);
      _mm_stream_si128(reinterpret_cast<__m128i *>(dst) + 4 * i + 1, b);
      _mm_stream_si128(reinterpret_cast<__m128i *>(dst) + 4 * i + 2, c);
      _mm_stream_si128(reinterpret_cast<__m128i *>(dst) + 4 * i + 3, d);
    }
    _mm_sfence();  // the stores are globally visible before the message is queued
    if (bytes % 64) memcpy(dst + blocks * 64, src + blocks * 64, bytes % 64);
    return;
  }
#endif
  memcpy(dst, src, bytes);
}

static size_t bytesPerSample(SampleQueue::SampleKind k) {
  switch (k) {
    case SampleQueue::ByteComplex: return 2;
    case SampleQueue::Short:
    case SampleQueue::ShortComplex: return 4;
    case SampleQueue::FloatComplex: return 8;
    default: return 0;
  }
}

// The recycle ring holds bufferCount / 10 processed messages; capture needs some history to find the pre-trigger buffers in.
static size_t historyCapacity(uint32_t bufferCount, bool doWrite) {
  return doWrite && bufferCount / 10 < 8 ? 8 : bufferCount / 10;
}

SampleQueue::SampleQueue(SampleKind kind, uint32_t enob, uint32_t sampleCount, uint32_t bufferCount,
                         bool correctDCOffset, bool doWrite)
    : m_kind(kind), m_enob(enob), m_sampleCount(sampleCount), m_bufferCount(bufferCount),
      m_correctDCOffset(correctDCOffset), m_doWrite(doWrite), m_bufferBytes(bytesPerSample(kind) * sampleCount),
      m_writer(m_bufferBytes, sampleCount, kind == FloatComplex, historyCapacity(bufferCount, doWrite), doWrite) {
  assert(kind > Illegal && kind <= FloatComplex);  // messageQueue.h:163
  assert(bufferCount > 0);
  uint32_t poolSize = uint32_t(bufferCount * 1.1);
  if (poolSize <= bufferCount) poolSize = bufferCount + 1;
  if (historyCapacity(bufferCount, doWrite) > bufferCount / 10) poolSize += 8;  // (the history it was given on top)
  for (uint32_t i = 0; i < poolSize; i++) {
    m_pool.emplace_back(new MessageType(m_bufferBytes));
    m_free.push_back(m_pool.back().get());
  }
}

SampleQueue::~SampleQueue() {
  assert(m_buffer.empty() && m_rings.Queued() == 0);  // messageQueue.h:173
}

SampleQueue::MessageType *SampleQueue::Allocate() {  // memoryPool.h:60-68
  std::unique_lock<std::mutex> lock(m_poolMutex);
  while (m_free.empty()) m_poolNotEmpty.wait(lock);
  MessageType *m = m_free.front();
  m_free.pop_front();
  return m;
}

void SampleQueue::Free(MessageType *m) {  // memoryPool.h:69-76
  std::unique_lock<std::mutex> lock(m_poolMutex);
  bool wasEmpty = m_free.empty();
  m_free.push_back(m);
  if (wasEmpty) m_poolNotEmpty.notify_one();
}

void SampleQueue::WaitNotFull(Lock &lock) {
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  m_notFull.wait(lock);
  m_producerWaitNs += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}

// A place in a consumer's pinned slot: waits for room in the queue AND in a slot (stagingRings.h says which; consumers that take,
// release, attach or detach signal m_notFull).  The message object is the place's own.  nullptr once no ring is attached (never
// attached, or detached while waiting).
SampleQueue::MessageType *SampleQueue::WaitForPlace(Lock &lock) {
  StagingRings::Place p;
  while (m_rings.Attached()) {
    if (!m_rings.Acquire(HasRoom(), &p)) {
      WaitNotFull(lock);
      continue;
    }
    RingStorage &g = m_ringStorage[p.ring];
    MessageType *message = g.messages[(size_t)p.slot * m_rings.BuffersPerSlot() + p.index].get();
    message->m_ring = p.ring;
    message->m_slot = p.slot;
    message->m_staged = g.bases[p.slot] + (size_t)p.index * m_bufferBytes;
    return message;
  }
  return nullptr;
}

// The consumer may have attached its slots while `pooled` was being filled outside the lock: the buffer then takes a place in a
// slot like any later one (behind whatever was queued at the attach), so that from the attach on every NEW message is a staged
// one and the consumer never has to fit a copied message between slots the producer is writing to.  Returns the message to queue.
SampleQueue::MessageType *SampleQueue::MoveIntoSlotIfAttached(Lock &lock, MessageType *pooled) {
  while (!m_rings.Attached() && m_buffer.size() >= m_bufferCount) WaitNotFull(lock);  // (room in the queue first: an attach may come while waiting)
  MessageType *const staged = WaitForPlace(lock);
  if (!staged) return pooled;
  memcpy(staged->m_staged, pooled->GetRawData(), m_bufferBytes);
  Free(pooled);
  return staged;
}

void SampleQueue::SynchronizedAppend(const void *a, size_t aBytes, const void *b, size_t bBytes,
                                     double centerFrequency, time_t time) {
  // messageQueue.h:65-91
  if (time) m_iterationCount++;
  if (m_iterationCount < 2) return;  // the first (warm-up) sweep is discarded
  assert(aBytes + bBytes == m_bufferBytes);
  Lock lock(m_mutex);
  MessageType *message = WaitForPlace(lock);
  if (message) {
    // The copy runs under the queue's lock: the consumer seals a slot by what is QUEUED, so a buffer must not be half-way
    // into a slot when that happens (1.6 us for a 32 KiB buffer; the consumer takes a whole batch per lock round trip).
    stream_copy(message->m_staged, static_cast<const unsigned char *>(a), aBytes);
    if (bBytes) stream_copy(message->m_staged + aBytes, static_cast<const unsigned char *>(b), bBytes);
  } else {
    lock.unlock();
    message = Allocate();
    message->m_staged = nullptr;
    message->m_slot = -1;
    message->m_ring = -1;
    memcpy(message->GetRawData(), a, aBytes);
    if (bBytes) memcpy(static_cast<unsigned char *>(message->GetRawData()) + aBytes, b, bBytes);
    lock.lock();
    message = MoveIntoSlotIfAttached(lock, message);
  }
  const bool staged = message->m_ring >= 0;
  (staged ? m_stagedAppends : m_copiedAppends)++;
  MessageHeader &h = message->GetHeader();
  h.m_time = time;
  h.m_frequency = centerFrequency;
  h.m_kind = MessageHeader::ProcessData;
  h.m_referenceCount = 0;
  h.m_sequenceId = m_nextSequenceId++;
  if (staged) {  // (room in the queue was waited for when the place was taken)
    if (m_rings.MarkQueued(message->m_ring)) m_notEmpty.notify_all();  // (every consumer waits on the one condition, each for its own ring)
  } else {
    while (!HasRoom()) WaitNotFull(lock);
    const bool wake = m_buffer.empty();
    m_buffer.push_front(message);
    if (wake) m_notEmpty.notify_all();
  }
  ClearAck();
}

void SampleQueue::AppendSamples(int16_t *re, int16_t *im, double fc, time_t time) {
  assert(m_kind == Short);  // planar: I block then Q block (SCN_KIND_SHORT layout)
  SynchronizedAppend(re, 2 * (size_t)m_sampleCount, im, 2 * (size_t)m_sampleCount, fc, time);
}
void SampleQueue::AppendSamples(int16_t s[][2], double fc, time_t time) {
  assert(m_kind == ShortComplex);
  SynchronizedAppend(s, m_bufferBytes, nullptr, 0, fc, time);
}
void SampleQueue::AppendSamples(int8_t (*s)[2], double fc, time_t time) {
  assert(m_kind == ByteComplex);
  SynchronizedAppend(s, m_bufferBytes, nullptr, 0, fc, time);
}
void SampleQueue::AppendSamples(fftwf_complex *s, double fc, time_t time) {
  assert(m_kind == FloatComplex);
  SynchronizedAppend(s, m_bufferBytes, nullptr, 0, fc, time);
}

SampleQueue::MessageType *SampleQueue::PopOldest() {
  const bool wake = !HasRoom();
  MessageType *m = m_buffer.back();
  m_buffer.pop_back();
  m_rings.UnstagedTaken();  // (a consumer without a ring taking what was queued before the first attach)
  if (wake || m_rings.Attached()) m_notFull.notify_all();
  return m;
}

SampleQueue::MessageType *SampleQueue::GetNextSamples() {
  Lock lock(m_mutex);
  while (!m_done && m_buffer.empty()) m_notEmpty.wait(lock);
  return m_buffer.empty() ? nullptr : PopOldest();  // (nullptr: done and drained)
}

SampleQueue::MessageType *SampleQueue::TryGetNextSamples() {
  Lock lock(m_mutex);
  return m_buffer.empty() ? nullptr : PopOldest();
}

int SampleQueue::AttachStaging(void *const *slotBases, uint32_t nSlots, uint32_t buffersPerSlot) {
  if (m_doWrite) return -1;  // (the capture writer's history needs storage of its own)
  Lock lock(m_mutex);
  // The documented start order is Start, StartStreaming, THEN StartProcessing (signalSource.h:5, scan.cpp:234-238), and a plan
  // takes hundreds of milliseconds to create: the producer has almost always queued buffers by now, often a full queue of
  // them.  (Until round 5 a non-empty queue refused the attach -- silently, so the zero-copy path all but never engaged.)
  // Those messages stay what they are, pooled and unstaged; the consumers take them first (TakeStagedBatch).
  const bool first = !m_rings.Attached();  // the first consumer: from here on every NEW message is a staged one
  const int ring = m_rings.Attach(nSlots, buffersPerSlot, m_buffer.size());
  if (ring < 0) return -1;
  m_ringStorage.emplace_back();
  RingStorage &g = m_ringStorage.back();
  for (uint32_t i = 0; i < nSlots; i++) g.bases.push_back(static_cast<unsigned char *>(slotBases[i]));
  for (size_t i = 0; i < (size_t)nSlots * buffersPerSlot; i++) g.messages.emplace_back(new MessageType(0));
  if (first) m_queuedAtAttach = m_buffer.size();
  m_notFull.notify_all();  // (a producer waiting for a slot has one more ring to look at)
  return ring;
}

void SampleQueue::DetachStaging(int ring) {
  Lock lock(m_mutex);
  if (!m_rings.IsAttached(ring)) return;
  m_rings.Detach(ring);  // (a consumer that gives up: what it had queued lives in its plan's slots and goes with them)
  m_notFull.notify_all();  // a producer waiting for a slot goes on with another ring, or with the messages' own storage
  m_notEmpty.notify_all();
}

uint32_t SampleQueue::TakeStagedBatch(int ring, std::vector<MessageType *> &out, int *slot, bool block, uint32_t lingerMicros) {
  Lock lock(m_mutex);
  if (!m_rings.IsAttached(ring)) return 0;
  while (block && !m_done && !m_rings.Queued(ring) && !m_rings.Unstaged()) m_notEmpty.wait(lock);
  // An idle consumer woken by the first buffer of a burst lingers a moment before it seals the slot: taking that one
  // buffer at once would make the producer pay a futex wake for EVERY append (it signals whenever it finds the ring
  // empty: ~1 us per 32 KiB buffer, as much as the copy) and the GPU a launch per buffer.  A front-end that delivers a
  // buffer every 80 us is not held up: the wait ends after lingerMicros at the latest.
  if (block && lingerMicros && !m_done && !m_rings.Unstaged() && m_rings.Queued(ring) && m_rings.Queued(ring) < m_rings.BuffersPerSlot())
    m_notEmpty.wait_until(lock, std::chrono::system_clock::now() + std::chrono::microseconds(lingerMicros));  // (system clock -> pthread_cond_timedwait: gcc 11's TSan does not know the steady-clock wait)
  uint32_t n = 0;
  if (m_rings.Reserve(ring, slot, &n)) {  // messages queued before the attach, oldest first, and this ring's next slot to copy them into
    for (uint32_t i = 0; i < n; i++) {
      out.push_back(m_buffer.back());
      m_buffer.pop_back();
    }
  } else if (m_rings.Take(ring, slot, &n)) {
    RingStorage &g = m_ringStorage[ring];
    for (uint32_t i = 0; i < n; i++) out.push_back(g.messages[(size_t)*slot * m_rings.BuffersPerSlot() + i].get());
  } else {
    return 0;
  }
  m_notFull.notify_all();
  return n;
}

void SampleQueue::ReleaseStaging(int ring, int slot) {
  Lock lock(m_mutex);
  m_rings.Release(ring, slot);
  m_notFull.notify_all();
}

void SampleQueue::MessageProcessed(MessageType *message) {
  assert(message->GetHeader().m_kind != MessageHeader::Illegal);
  if (message->m_staged) {  // its samples live in the consumer's slot, which is about to be refilled, and so does the
    message->m_header.m_kind = MessageHeader::Free;  // message object itself: nothing to keep, nothing to recycle
    return;
  }
  if (MessageType *recycled = m_writer.Keep(message)) Free(recycled);
}

void SampleQueue::SetIsDone() {
  {
    Lock lock(m_mutex);
    assert(!m_done);
    m_done = true;
    m_notEmpty.notify_all();
  }
  m_writer.Wake();  // messageQueue.h:299-303: wake the writer too
}

bool SampleQueue::GetIsDone() {
  Lock lock(m_mutex);
  return m_done;
}

bool SampleQueue::ReceivedAck() { return m_acknowledged; }
void SampleQueue::SendAck() {
  bool expected = false;
  m_acknowledged.compare_exchange_strong(expected, true);
}
void SampleQueue::ClearAck() {
  bool expected = true;
  m_acknowledged.compare_exchange_strong(expected, false);
}
