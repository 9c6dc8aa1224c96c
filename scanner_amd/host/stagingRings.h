// stagingRings.h -- the state machine of SampleQueue's zero-copy staging, and nothing else: no lock, no wait, no clock, no copy,
// no message.  It deals in PLACES (ring, slot, index) and counts; SampleQueue (messageQueue.h) calls it under its mutex and keeps
// the waiting, the memory behind the places and the message objects.
//
// Every consumer thread lends the queue the pinned submit slots of its scn_plan as a RING of its own (Attach).  The producer then
// writes a buffer straight into the next free place of the slot being filled (Acquire, then MarkQueued once the samples are in),
// and the consumer submits a slot as it is: Take hands out every queued place of that consumer's oldest slot (places 0 .. n-1 of
// it, in order) and seals the slot, so that the producer moves on; the slot returns to the producer with Release, after the
// consumer has collected its results.  A slot: Free -> Open (being filled / holding queued places) -> InFlight (taken) -> Free.
// With several consumers (scan.cpp:217 runs two) the producer deals its batches round-robin: when the slot it is filling is full
// or has been sealed it goes on to the NEXT consumer's ring that has a usable slot -- the ring's fill slot if that is free or open
// with room, or the one after it once the fill slot is full and still queued.  Within a ring the producer opens, and the consumer
// therefore seals, slots strictly in ring order: the order the consumer submits its slots in.
//
// Messages that were queued before the first attach (the producer runs while the consumers are still creating their plans) stay
// what they are, pooled and unstaged.  They are handed out first, a slot's worth at a time, together with the asking consumer's
// next slot in ring order reserved for them (Reserve: the consumer copies those itself), and the producer opens no slot while one
// of them is left: at no time do a consumer's copy and the producer's append write to the same slot, and nothing is reordered.
//
// The callers' part of the contract: MarkQueued follows its Acquire before any other call (the queue copies under its lock); a
// consumer takes or reserves only while it holds fewer slots than its ring has, and releases the slots it holds oldest first.
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>
#include <vector>

class StagingRings {
 public:
  struct Place {
    int ring, slot;
    uint32_t index;  // the buffer's position in the slot
  };

  // A consumer's ring of nSlots slots of buffersPerSlot places each; `queuedUnstaged` is what the queue holds right now.  Returns
  // the ring's id (>= 0; ids are never reused), or -1: fewer than two slots, no places, or a batch size other than that of the
  // rings already attached (one for all the consumers of a queue).  The first ring attached makes everything queued so far the
  // unstaged backlog, and every NEW buffer a staged one.
  int Attach(uint32_t nSlots, uint32_t buffersPerSlot, size_t queuedUnstaged) {
    if (nSlots < 2 || buffersPerSlot == 0 || (m_attached && buffersPerSlot != m_buffersPerSlot)) return -1;
    m_rings.push_back(Ring{std::vector<Slot>(nSlots, Slot{Slot::Free, 0}), 0, 0, true});
    if (!m_attached++) {
      m_buffersPerSlot = buffersPerSlot;
      m_unstaged = queuedUnstaged;
      m_fillRing = (int)m_rings.size() - 1;
    }
    return (int)m_rings.size() - 1;
  }

  // The consumer is leaving.  Returns how many queued places go with the ring (they live in its plan's slots); the ring yields
  // nothing from here on.  With the last ring gone there is no backlog any more: whoever is left takes the queue the plain way.
  size_t Detach(int ring) {
    if (!IsAttached(ring)) return 0;
    Ring &g = m_rings[ring];
    const size_t dropped = g.queued;
    g.attached = false;
    g.queued = 0;
    m_queued -= dropped;
    if (!--m_attached) m_unstaged = 0;
    return dropped;
  }

  // The producer's next place; false if there is none: no ring attached, a backlog left, no room in the queue (`room`: the bound
  // is the queue's, staged and pooled messages together), or every attached ring's next slot still in flight.  The batch in
  // progress goes on in its slot while that is open and has room; a new batch starts in the next attached ring, round-robin,
  // that has a usable slot.  The one function that moves the fill ring and a ring's fill slot forward for the producer.
  bool Acquire(bool room, Place *place) {
    if (!m_attached || m_unstaged || !room) return false;
    const int R = (int)m_rings.size();
    int ring = -1, slot = -1;
    const Ring &cur = m_rings[m_fillRing];
    if (cur.attached && cur.slots[cur.fillSlot].state == Slot::Open && cur.slots[cur.fillSlot].fill < m_buffersPerSlot) {
      ring = m_fillRing;
      slot = cur.fillSlot;
    }
    for (int k = 1; ring < 0 && k <= R; k++) {  // a new batch: the next consumer's turn
      const int r = (m_fillRing + k) % R;
      if (m_rings[r].attached && (slot = UsableSlot(m_rings[r])) >= 0) ring = r;
    }
    if (ring < 0) return false;
    m_fillRing = ring;
    m_rings[ring].fillSlot = slot;
    Slot &s = m_rings[ring].slots[slot];
    if (s.state == Slot::Free) {
      s.state = Slot::Open;
      s.fill = 0;
    }
    *place = Place{ring, slot, s.fill++};
    return true;
  }

  // The samples are in the place Acquire gave out last, in `ring`.  True if the ring had nothing queued: its consumer may be asleep.
  bool MarkQueued(int ring) {
    m_queued++;
    return !m_rings[ring].queued++;
  }

  // The ring's oldest slot with its `count` queued places, 0 .. count - 1; false if the ring has nothing queued (or is detached).
  // Taking seals the slot, full or not: the producer moves on, past it if it was the fill slot.
  bool Take(int ring, int *slot, uint32_t *count) {
    if (!IsAttached(ring) || !m_rings[ring].queued) return false;
    Ring &g = m_rings[ring];
    const int n = (int)g.slots.size();
    int s = g.fillSlot;  // the open slots are a run in ring order that ends at the fill slot: the oldest is its first
    for (int back = 1; back < n && g.slots[(s + n - 1) % n].state == Slot::Open; back++) s = (s + n - 1) % n;
    *slot = s;
    *count = g.slots[s].fill;
    g.slots[s].state = Slot::InFlight;
    g.queued -= *count;
    m_queued -= *count;
    if (s == g.fillSlot) g.fillSlot = (s + 1) % n;
    return true;
  }

  // The ring's next slot, reserved (in flight) for up to a slot's worth of the backlog, oldest first: `count` messages the caller
  // takes from the queue and copies into the slot itself.  False if there is no backlog (or the ring is detached).
  bool Reserve(int ring, int *slot, uint32_t *count) {
    if (!IsAttached(ring) || !m_unstaged) return false;
    Ring &g = m_rings[ring];
    *slot = g.fillSlot;
    *count = m_unstaged < m_buffersPerSlot ? (uint32_t)m_unstaged : m_buffersPerSlot;
    m_unstaged -= *count;
    g.slots[g.fillSlot] = Slot{Slot::InFlight, 0};
    g.fillSlot = (g.fillSlot + 1) % (int)g.slots.size();
    return true;
  }

  // One message of the backlog left the queue the plain way (a consumer without a ring).
  void UnstagedTaken() {
    if (m_unstaged) m_unstaged--;
  }

  // The consumer has collected the slot's results: it is the producer's again (a detached ring's slots may still come back).
  void Release(int ring, int slot) {
    if (ring >= 0 && (size_t)ring < m_rings.size() && slot >= 0 && (size_t)slot < m_rings[ring].slots.size())
      m_rings[ring].slots[slot].state = Slot::Free;
  }

  bool IsAttached(int ring) const { return ring >= 0 && (size_t)ring < m_rings.size() && m_rings[ring].attached; }
  uint32_t Attached() const { return m_attached; }                     // rings
  size_t Queued() const { return m_queued; }                           // places queued in all the rings: they count towards the queue's bound
  size_t Queued(int ring) const { return m_rings[ring].queued; }       // (an attached ring's)
  size_t Unstaged() const { return m_unstaged; }                       // the backlog no consumer has taken yet: the oldest in the queue
  uint32_t BuffersPerSlot() const { return m_buffersPerSlot; }         // the same for every ring: the consumers' batch size

 private:
  struct Slot {
    enum State { Free, Open, InFlight } state;
    uint32_t fill;  // places handed out since the slot was opened
  };
  struct Ring {  // one per consumer; entries stay (detached) for good, so that an id names one ring for ever
    std::vector<Slot> slots;
    size_t queued;  // places marked queued and not yet taken: all of every open slot's but, between Acquire and MarkQueued, the last
    int fillSlot;   // the slot the producer fills next in this ring
    bool attached;
  };

  // The slot of `g` a new batch may start or go on in, -1 if there is none: the fill slot if it is free, or open with room; the one
  // after it if the fill slot is full and still queued and that one is free (in flight, it is next in submit order: wait for it).
  int UsableSlot(const Ring &g) const {
    const Slot &fs = g.slots[g.fillSlot];
    if (fs.state == Slot::Free || (fs.state == Slot::Open && fs.fill < m_buffersPerSlot)) return g.fillSlot;
    const int next = (g.fillSlot + 1) % (int)g.slots.size();
    return fs.state == Slot::Open && g.slots[next].state == Slot::Free ? next : -1;
  }

  std::deque<Ring> m_rings;  // index = ring id
  uint32_t m_attached = 0, m_buffersPerSlot = 0;
  int m_fillRing = 0;        // the ring whose slot the producer is filling
  size_t m_queued = 0, m_unstaged = 0;
};
