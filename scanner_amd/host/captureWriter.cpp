#include "captureWriter.h"

#include <cstring>
#include <limits>
#include <vector>

CaptureWriter::CaptureWriter(size_t bufferBytes, uint32_t sampleCount, bool rawIsFloat, size_t historyCapacity, bool doWrite)
    : m_bufferBytes(bufferBytes), m_historyCapacity(historyCapacity), m_sampleCount(sampleCount), m_rawIsFloat(rawIsFloat),
      m_doWrite(doWrite) {
  if (m_doWrite) {
    printf("Starting write thread...\n");  // messageQueue.h:166
    m_thread.reset(new std::thread(&CaptureWriter::WriteThreadWorker, this));
  }
}

CaptureWriter::~CaptureWriter() {
  if (!m_thread) return;  // (no thread, no job: BeginWrite opens a file only for a writer that writes)
  printf("Stopping write thread...\n");  // messageQueue.h:176
  {
    std::unique_lock<std::mutex> lock(m_mutex);
    m_shutdown = true;
    m_writeWake.notify_all();
  }
  m_thread->join();
}

SampleMessage *CaptureWriter::Keep(SampleMessage *message) {
  if (m_historyCapacity == 0) return message;  // (the reference's zero-capacity ring would misbehave; recycle at once)
  std::unique_lock<std::mutex> lock(m_mutex);
  SampleMessage *old = nullptr;
  if (m_history.size() >= m_historyCapacity) {
    // Back-pressure the reference lacks: the oldest message is not recycled while the capture
    // writer still has to dump it (the reference silently loses records when its ring laps the writer).
    while (!m_history.empty() && WriterNeeds(m_history.back()->GetHeader().m_sequenceId)) {
      m_writeWake.notify_one();
      m_writeDrained.wait(lock);
    }
    old = m_history.back();
    m_history.pop_back();
  }
  m_history.push_front(message);
  if (!m_captures.empty()) m_writeWake.notify_one();  // messageQueue.h:272
  return old;
}

bool CaptureWriter::WriterNeeds(uint64_t sequenceId) const {
  for (const CaptureJob &job : m_captures)
    if (sequenceId >= job.next && sequenceId < job.end) return true;
  return false;
}

void CaptureWriter::SetConverter(Converter c) {
  std::unique_lock<std::mutex> lock(m_mutex);
  m_converter = c;
}

void CaptureWriter::CloseNewestAt(uint64_t sequenceId) {
  if (!m_captures.empty() && m_captures.back().open) {
    m_captures.back().end = sequenceId;
    m_captures.back().open = false;
  }
}

void CaptureWriter::BeginWrite(uint64_t startSequenceId, std::string fileName) {
  printf("BeginWrite %s: %lu\n", fileName.c_str(), (unsigned long)startSequenceId);  // messageQueue.h:276
  FILE *file = nullptr;
  if (m_doWrite) {
    file = fopen(fileName.c_str(), "w");
    if (!file) {
      fprintf(stderr, "Failed to open file '%s'\n", fileName.c_str());
      m_writeErrors++;
    }
  }
  std::unique_lock<std::mutex> lock(m_mutex);
  m_writeStart = startSequenceId;
  m_writeEnd = std::numeric_limits<uint64_t>::max();
  CloseNewestAt(startSequenceId);  // a capture still waiting for its EndWrite when the next trigger begins ends where the new one starts
  if (file) {
    m_captures.push_back(CaptureJob{file, startSequenceId, m_writeEnd, true});
    m_writeWake.notify_one();
  }
}

void CaptureWriter::EndWrite(uint64_t sequenceId) {
  printf("EndWrite %lu\n", (unsigned long)sequenceId);  // messageQueue.h:285
  std::unique_lock<std::mutex> lock(m_mutex);
  m_writeEnd = sequenceId;
  // only the job the matching BeginWrite queued gets its end: if that BeginWrite queued nothing (writing switched off, or
  // its file could not be opened) the newest job belongs to an EARLIER trigger whose end is already fixed -- leave it alone
  CloseNewestAt(sequenceId);
  m_writeWake.notify_one();
}

void CaptureWriter::Wake() {
  std::unique_lock<std::mutex> lock(m_mutex);
  m_writeWake.notify_all();
}

// messageQueue.h:98-139 restated as a job loop: for the oldest queued capture write, in sequence order, every
// processed message with an id in [next, end) as it reaches the history ring; the job is finished -- and its file
// closed, by this thread only -- once a message at or past its end id (or the end of the stream) shows up.
void CaptureWriter::WriteThreadWorker() {
  std::vector<unsigned char> raw(m_bufferBytes);
  std::vector<float> converted(2 * (size_t)m_sampleCount);
  std::unique_lock<std::mutex> lock(m_mutex);
  while (true) {
    // (the reference's writer gives up as soon as the PRODUCER is done, messageQueue.h:100-121, losing
    // whatever the consumers had not processed yet; this one runs until the queue is torn down)
    while (!m_shutdown && m_captures.empty()) m_writeWake.wait(lock);
    if (m_captures.empty()) break;  // shutting down, nothing being written
    CaptureJob &job = m_captures.front();
    // oldest -> newest: find the first message this capture still wants
    SampleMessage *next = nullptr;
    bool pastEnd = false;
    for (auto it = m_history.rbegin(); it != m_history.rend(); ++it) {
      const uint64_t seq = (*it)->GetHeader().m_sequenceId;
      if (seq < job.next) continue;
      if (seq >= job.end) {
        pastEnd = true;
      } else {
        next = *it;
      }
      break;
    }
    if (next) {
      const uint64_t seq = next->GetHeader().m_sequenceId;
      memcpy(raw.data(), next->GetRawData(), m_bufferBytes);
      job.next = seq + 1;  // the ring may recycle the message from here on
      FILE *const file = job.file;  // stays open: only this thread closes it, and only after this record
      const Converter convert = m_converter;
      lock.unlock();
      printf("Writing %lu\n", (unsigned long)seq);  // messageQueue.h:125
      const void *data = raw.data();
      size_t bytes = m_bufferBytes;
      if (!m_rawIsFloat) {
        if (convert) {
          convert(raw.data(), 1, converted.data());
          data = converted.data();
          bytes = sizeof(fftwf_complex) * m_sampleCount;
        } else {
          fprintf(stderr, "SampleQueue: no converter installed, writing raw samples\n");
        }
      }
      if (fwrite(data, 1, bytes, file) != bytes) m_writeErrors++;
      lock.lock();
      m_writeDrained.notify_all();
      continue;
    }
    if (pastEnd || m_shutdown) {  // capture complete (or the queue is going away): close its file
      fclose(job.file);
      m_captures.pop_front();
      m_writeDrained.notify_all();
      continue;
    }
    m_writeWake.wait(lock);
  }
}
