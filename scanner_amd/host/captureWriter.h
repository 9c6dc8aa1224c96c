// captureWriter.h -- CaptureWriter: the recycle ring of processed messages and the triggered capture that reads it
// (messageQueue.h:98-139, 259-288).  SampleQueue hands every processed pooled message to Keep and recycles what Keep hands back;
// with doWrite a write thread dumps the kept messages with sequence ids in [start, end) to the capture's file as raw
// little-endian fftwf_complex[sampleCount] records -- the reference's file format.  Messages hold raw wire-format samples, so
// integer kinds go through the converter (K1 on the GPU, scn_convert_raw) that the consumer installs.
//
// Captures are jobs the write thread owns: BeginWrite opens the file and queues {file, [start, end)}, EndWrite fixes the end of
// the newest job, and the writer alone writes to and closes each file once it has dumped the job's last record -- so a re-trigger
// while the previous capture is still draining (a record costs a GPU round trip for the integer formats) starts a second job
// instead of closing a file in use.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "sampleMessage.h"

class CaptureWriter {
 public:
  typedef std::function<void(const void *raw, uint32_t nBuffers, float *out)> Converter;

  // The messages are the caller's: they must outlive the writer, which reads them until it is destroyed.
  CaptureWriter(size_t bufferBytes, uint32_t sampleCount, bool rawIsFloat, size_t historyCapacity, bool doWrite);
  ~CaptureWriter();  // drains the captures that are queued, closes their files and joins the write thread

  // Keeps a processed message for the captures to come; returns the message that leaves the ring for it -- the oldest, once the
  // ring is full and no capture needs it any more (this blocks while one does) -- or nullptr.
  SampleMessage *Keep(SampleMessage *message);

  void BeginWrite(uint64_t startSequenceId, std::string fileName);
  void EndWrite(uint64_t sequenceId);
  void SetConverter(Converter c);  // install before the consumers start; the writer calls a copy taken under the lock
  void Wake();                     // the producer is done (messageQueue.h:299-303)

  uint64_t GetWriteStartSequenceId() const { return m_writeStart; }
  uint64_t GetWriteEndSequenceId() const { return m_writeEnd; }
  uint32_t GetWriteErrorCount() const { return m_writeErrors; }  // files that could not be opened / short writes

 private:
  struct CaptureJob {
    FILE *file;
    uint64_t next, end;  // the writer still owes the records with ids in [next, end)
    bool open;           // its EndWrite has not come yet: `end` is still the placeholder
  };
  void WriteThreadWorker();
  bool WriterNeeds(uint64_t sequenceId) const;  // some queued capture has not dumped this record yet
  void CloseNewestAt(uint64_t sequenceId);      // the newest job, if it still waits for its end, ends here

  const size_t m_bufferBytes, m_historyCapacity;
  const uint32_t m_sampleCount;
  const bool m_rawIsFloat, m_doWrite;
  // everything below is guarded by m_mutex (the atomic is also read without it)
  std::mutex m_mutex;
  std::condition_variable m_writeWake, m_writeDrained;
  std::deque<SampleMessage *> m_history;  // processed messages kept for capture, front = newest
  std::deque<CaptureJob> m_captures;      // front = the one being written
  uint64_t m_writeStart = 0, m_writeEnd = 0;  // bounds of the newest capture (the reference's two fields, messageQueue.h:52-53)
  bool m_shutdown = false;  // set by the destructor: the consumers are gone, drain what is there and stop
  std::atomic<uint32_t> m_writeErrors{0};
  Converter m_converter;
  std::unique_ptr<std::thread> m_thread;
};
