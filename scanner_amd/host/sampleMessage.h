// sampleMessage.h -- what travels through a SampleQueue: a header and the RAW device-format samples of one buffer.  At namespace
// scope so that the capture writer (captureWriter.h) can name them; SampleQueue::MessageType and SampleQueue::MessageHeader are
// these two.
#pragma once
#include <cstddef>
#include <cstdint>
#include <ctime>
#include <vector>

#include "scannerCompat.h"

struct SampleMessageHeader {  // messageQueue.h:15-28
  enum MessageKind { Illegal = 0, ProcessData, WriteData, WriteDataAndStop, Free } m_kind;
  uint32_t m_referenceCount;
  double m_frequency;
  uint64_t m_sequenceId;
  time_t m_time;
};

class SampleMessage {  // Buffer<MessageHeader, T> of memoryPool.h:7-30
 public:
  SampleMessageHeader m_header;
  explicit SampleMessage(size_t bytes) : m_header(), m_raw(bytes), m_staged(nullptr), m_slot(-1), m_ring(-1) {}
  SampleMessageHeader &GetHeader() { return m_header; }
  void *GetRawData() { return m_staged ? static_cast<void *>(m_staged) : static_cast<void *>(m_raw.data()); }
  size_t GetRawBytes() const { return m_raw.size(); }
  // Valid for FloatComplex queues only (raw == converted); integer kinds are converted on the GPU.
  fftwf_complex *GetData() { return reinterpret_cast<fftwf_complex *>(GetRawData()); }
  int GetStagingSlot() const { return m_slot; }  // -1: the samples live in the message itself

 private:
  friend class SampleQueue;
  std::vector<unsigned char> m_raw;
  unsigned char *m_staged;  // staged queues: the samples' place in the consumer's pinned submit slot (AttachStaging)
  int m_slot, m_ring;
};
