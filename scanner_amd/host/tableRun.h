// tableRun.h -- which run of the sweep's frequency table a batch of centre frequencies is (ProcessSamples::SetFrequencyTable): a
// cursor over the table.  A batch that is a consecutive, wrapping run of it is submitted by naming its first entry.
#pragma once
#include <cstdint>
#include <vector>

class TableRun {
 public:
  explicit TableRun(const std::vector<double> &table) : m_table(table), m_next(0) {}

  // True, with *first the entry the run starts at, if f[0 .. n) is a run of the table: from where the last run ended or, failing
  // that, from the FIRST entry equal to f[0] (no second candidate is tried).  A run may wrap any number of times; a batch that is
  // no run leaves the cursor where it was.
  bool Run(const std::vector<double> &f, uint32_t n, uint32_t *first) {
    const uint32_t count = (uint32_t)m_table.size();
    if (!count) return false;
    uint32_t at = m_next;
    if (m_table[at] != f[0]) {  // (another consumer took the batches in between, or the stream started mid-table: look it up)
      at = 0;
      while (at < count && m_table[at] != f[0]) at++;
      if (at == count) return false;
    }
    for (uint32_t b = 0; b < n; b++)
      if (m_table[(at + b) % count] != f[b]) return false;
    *first = at;
    m_next = (at + n) % count;
    return true;
  }

 private:
  const std::vector<double> &m_table;
  uint32_t m_next;  // where the run is expected to go on
};
