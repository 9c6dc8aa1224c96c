// messageQueue.h -- SampleQueue: the bounded producer/consumer queue between a SignalSource
// and ProcessSamples.  Same public surface as the reference's MessageQueue<fftwf_complex>
// (messageQueue.h:141-324) with one deliberate change of representation: a message holds the
// RAW device-format samples (int8 / int16 / float IQ), not converted floats -- the
// int->float convert (utility.cpp:9-84) runs on the GPU inside the fused kernel, so the
// producer thread no longer does arithmetic (the reference converts in AppendSamples,
// messageQueue.h:190-229).  Sequence ids, the discarded warm-up sweep, blocking behaviour,
// the ack bit and the recycle ring follow the reference.
//
// Three parts: this class is the reference's bounded queue and memory pool, with the lock, every wait and every copy;
// StagingRings (stagingRings.h) decides where a zero-copy append goes; CaptureWriter (captureWriter.h) keeps the processed
// messages and writes the triggered captures.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <ctime>
#include <deque>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "captureWriter.h"
#include "sampleMessage.h"
#include "scannerCompat.h"
#include "stagingRings.h"

class SampleQueue {
 public:
  typedef SampleMessageHeader MessageHeader;
  typedef SampleMessage MessageType;
  enum SampleKind { Illegal = 0, ByteComplex, Short, ShortComplex, FloatComplex };  // messageQueue.h:31-37

  SampleKind m_kind;

  SampleQueue(SampleKind kind, uint32_t enob, uint32_t sampleCount, uint32_t bufferCount, bool correctDCOffset,
              bool doWrite);
  ~SampleQueue();

  // messageQueue.h:190-237 (the four wire formats of the device front-ends)
  void AppendSamples(int16_t *realSamples, int16_t *imagSamples, double centerFrequency, time_t time);
  void AppendSamples(int16_t shortComplexSamples[][2], double centerFrequency, time_t time);
  void AppendSamples(int8_t (*byteComplexSamples)[2], double centerFrequency, time_t time);
  void AppendSamples(fftwf_complex *floatComplexSamples, double centerFrequency, time_t time);

  MessageType *GetNextSamples();     // blocking; nullptr once done and empty (messageQueue.h:239-257)
  MessageType *TryGetNextSamples();  // non-blocking variant used to fill a batch; nullptr if empty
  void MessageProcessed(MessageType *message);  // messageQueue.h:259-273

  // Triggered capture (messageQueue.h:98-139, 275-288), the CaptureWriter's: with doWrite the processed messages with sequence
  // ids in [start, end) go to `fileName`, through the converter the consumer installs for the integer kinds.
  void BeginWrite(uint64_t startSequenceId, std::string fileName) { m_writer.BeginWrite(startSequenceId, fileName); }
  void EndWrite(uint64_t sequenceId) { m_writer.EndWrite(sequenceId); }
  typedef CaptureWriter::Converter Converter;
  void SetConverter(Converter c) { m_writer.SetConverter(c); }  // install before the consumers start

  // Zero-copy staging (sampleBuffer.cpp's host staging "replaced by pinned double-buffered hipMemcpyAsync", BASELINE.json): every
  // consumer thread lends the queue the pinned submit slots of its scn_plan (scn_host_buffer) as a ring of its own, AppendSamples
  // writes a buffer straight into a slot -- the producer's one copy lands in pinned memory -- and the consumer submits the slot as
  // it is: TakeStagedBatch hands out the queued messages of the ring's oldest slot and seals it, ReleaseStaging gives the slot back
  // once its results are collected.  Which place an append goes to, in which order slots are sealed and how what was queued before
  // the first attach is handed out (unstaged, with a slot reserved: the consumer copies those itself) is stagingRings.h.  Sequence
  // ids are the queue's own, in append order; the discarded warm-up sweep (messageQueue.h:67-72), the queue's bound and its
  // blocking behaviour are unchanged.  A staged message is recycled as soon as it is processed: the capture writer's history needs
  // storage of its own, so a queue built with doWrite refuses staging and keeps the copying path.
  // AttachStaging returns the consumer's ring id (>= 0), or -1 when staging is refused.
  int AttachStaging(void *const *slotBases, uint32_t nSlots, uint32_t buffersPerSlot);
  void DetachStaging(int ring);  // the consumer is leaving; with the last ring gone appends fall back to the messages' own storage
  uint32_t TakeStagedBatch(int ring, std::vector<MessageType *> &out, int *slot, bool block, uint32_t lingerMicros = 0);
  void ReleaseStaging(int ring, int slot);

  void SetIsDone();
  bool GetIsDone();
  bool ReceivedAck();
  void SendAck();
  void ClearAck();

  // what a consumer needs to create its scn_plan
  uint32_t GetEnob() const { return m_enob; }
  uint32_t GetSampleCount() const { return m_sampleCount; }
  bool GetCorrectDCOffset() const { return m_correctDCOffset; }
  size_t GetBufferBytes() const { return m_bufferBytes; }
  uint32_t GetBufferCount() const { return m_bufferCount; }
  uint64_t GetWriteStartSequenceId() const { return m_writer.GetWriteStartSequenceId(); }
  uint64_t GetWriteEndSequenceId() const { return m_writer.GetWriteEndSequenceId(); }
  uint32_t GetWriteErrorCount() const { return m_writer.GetWriteErrorCount(); }  // files that could not be opened / short writes
  // seconds the producer has spent blocked in AppendSamples (queue full / no free staging slot): where a slow pipeline shows
  double GetProducerWaitSeconds() const { return m_producerWaitNs.load() * 1e-9; }
  // which path the appends took: written straight into a consumer's pinned slot / copied into a pooled message; and how many
  // messages were already queued when the consumer attached (the producer runs while the consumer is still creating its plan)
  uint64_t GetStagedAppendCount() const { return m_stagedAppends.load(); }
  uint64_t GetCopiedAppendCount() const { return m_copiedAppends.load(); }
  uint64_t GetQueuedAtAttachCount() const { return m_queuedAtAttach.load(); }

 private:
  typedef std::unique_lock<std::mutex> Lock;
  void SynchronizedAppend(const void *a, size_t aBytes, const void *b, size_t bBytes, double centerFrequency,
                          time_t time);
  void WaitNotFull(Lock &lock);                                   // one m_notFull wait, timed into m_producerWaitNs
  MessageType *WaitForPlace(Lock &lock);                          // the message of the producer's next staged place; nullptr: no ring attached
  MessageType *MoveIntoSlotIfAttached(Lock &lock, MessageType *pooled);
  MessageType *PopOldest();                                       // m_mutex held, m_buffer not empty
  bool HasRoom() const { return m_buffer.size() + m_rings.Queued() < m_bufferCount; }  // the bound: staged and pooled together
  MessageType *Allocate();
  void Free(MessageType *m);

  const uint32_t m_enob, m_sampleCount, m_bufferCount;
  const bool m_correctDCOffset, m_doWrite;
  const size_t m_bufferBytes;

  // the memory pool (memoryPool.h:32-77), 1.1 x depth plus the writer's history: it owns every pooled message
  std::vector<std::unique_ptr<MessageType>> m_pool;
  std::mutex m_poolMutex;
  std::condition_variable m_poolNotEmpty;
  std::list<MessageType *> m_free;

  // the queue (guarded by m_mutex)
  std::mutex m_mutex;
  std::condition_variable m_notEmpty, m_notFull;
  std::deque<MessageType *> m_buffer;  // pooled messages; front = newest (push_front / pop_back like the reference)
  uint64_t m_nextSequenceId = 0;
  uint32_t m_iterationCount = 0;  // (the producer's own)
  std::atomic<bool> m_done{false};
  std::atomic<bool> m_acknowledged{true};

  // staging (guarded by m_mutex): the state machine, and per ring the memory and the message objects behind its places
  struct RingStorage {
    std::vector<unsigned char *> bases;                  // [slot]
    std::vector<std::unique_ptr<MessageType>> messages;  // [slot][place]: headers only, so a staged buffer costs no pool round trip
  };
  StagingRings m_rings;
  std::deque<RingStorage> m_ringStorage;  // index = ring id; entries stay until the queue goes (a consumer may still hold messages)

  std::atomic<uint64_t> m_producerWaitNs{0}, m_stagedAppends{0}, m_copiedAppends{0}, m_queuedAtAttach{0};

  CaptureWriter m_writer;  // after m_pool: it reads the messages it keeps until it is destroyed
};
