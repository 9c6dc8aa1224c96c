// StagingRings (scanner_amd/host/stagingRings.h) alone: no queue, no thread, nothing of the project linked.
//  a. the scenario of test_staging_rings (test_host_cpu.cpp) restated on the core, place for place;
//  b. a fixed-seed walk of several hundred thousand operations against a model that is written here and shares no code with the
//     header: a flat record of who holds every place and every slot, from which the model works out what each call must answer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "stagingRings.h"

static uint64_t g_step = 0;
#define REQUIRE(c)                                                                               \
  do {                                                                                           \
    if (!(c)) {                                                                                  \
      fprintf(stderr, "FAIL %s:%d (step %llu): %s\n", __FILE__, __LINE__, (unsigned long long)g_step, #c); \
      exit(1);                                                                                   \
    }                                                                                            \
  } while (0)

typedef StagingRings::Place Place;

static bool acquireIs(StagingRings &s, int ring, int slot, uint32_t index) {
  Place p;
  if (!s.Acquire(true, &p) || p.ring != ring || p.slot != slot || p.index != index) return false;
  s.MarkQueued(p.ring);
  return true;
}
static bool takeIs(StagingRings &s, int ring, int slot, uint32_t count) {
  int sl = -1;
  uint32_t n = 0;
  return s.Take(ring, &sl, &n) && sl == slot && n == count;
}
static bool takesNothing(StagingRings &s, int ring) {
  int sl = -1;
  uint32_t n = 0;
  return !s.Take(ring, &sl, &n) && !s.Reserve(ring, &sl, &n);
}

// two rings of two slots of three places; two messages queued before the first attach
static void scripted() {
  StagingRings s;
  Place p;
  int slot = -1;
  uint32_t n = 0;
  REQUIRE(!s.Acquire(true, &p) && s.Attached() == 0);
  REQUIRE(s.Attach(2, 3, 2) == 0 && s.Attach(2, 3, 2) == 1 && s.Unstaged() == 2 && s.Attached() == 2 && s.BuffersPerSlot() == 3);
  REQUIRE(s.Attach(2, 4, 2) == -1 && s.Attach(1, 3, 2) == -1 && s.Attach(2, 0, 2) == -1);  // one batch size for all; two slots at least
  REQUIRE(!s.Acquire(true, &p));  // the producer opens no slot while the backlog is there
  // the unstaged ones first: whoever asks gets them with its next slot reserved
  REQUIRE(s.Reserve(1, &slot, &n) && slot == 0 && n == 2 && s.Unstaged() == 0);
  REQUIRE(takesNothing(s, 0));
  // batches of three go to the rings in turn -- a new batch starts in the ring AFTER the one filled last: ring 1 first (its slot 0
  // is reserved: slot 1), then ring 0, then -- ring 1 having no usable slot -- ring 0 again
  REQUIRE(acquireIs(s, 1, 1, 0) && acquireIs(s, 1, 1, 1) && acquireIs(s, 1, 1, 2));
  REQUIRE(acquireIs(s, 0, 0, 0) && acquireIs(s, 0, 0, 1) && acquireIs(s, 0, 0, 2));
  REQUIRE(acquireIs(s, 0, 1, 0));
  REQUIRE(s.Queued() == 7 && s.Queued(0) == 4 && s.Queued(1) == 3);
  REQUIRE(!s.Acquire(false, &p));  // the queue's bound
  REQUIRE(takeIs(s, 1, 1, 3));
  REQUIRE(takeIs(s, 0, 0, 3));
  REQUIRE(takeIs(s, 0, 1, 1));  // a partial batch, sealed by being taken
  REQUIRE(s.Queued() == 0);
  // ring 0: slot 0 in flight (never released), slot 1 just sealed; ring 1: slot 0 reserved, slot 1 in flight -> nothing usable
  REQUIRE(!s.Acquire(true, &p));
  s.Release(1, 0);
  REQUIRE(acquireIs(s, 1, 0, 0));
  REQUIRE(acquireIs(s, 1, 0, 1));  // the batch in progress goes on in the same slot
  REQUIRE(takesNothing(s, 0));
  REQUIRE(takeIs(s, 1, 0, 2));
  // a consumer that leaves takes its queued places with it; the other ring goes on
  s.Release(0, 0);
  REQUIRE(acquireIs(s, 0, 0, 0));
  REQUIRE(s.Detach(0) == 1 && s.Queued() == 0 && s.Attached() == 1 && !s.IsAttached(0));
  REQUIRE(takesNothing(s, 0));
  s.Release(1, 1);
  REQUIRE(acquireIs(s, 1, 1, 0));
  REQUIRE(takeIs(s, 1, 1, 1));
  // the last ring gone: no place any more
  REQUIRE(s.Detach(1) == 0 && s.Detach(1) == 0 && s.Attached() == 0);
  REQUIRE(!s.Acquire(true, &p));
  REQUIRE(s.Attach(3, 2, 5) == 2 && s.Unstaged() == 5 && s.BuffersPerSlot() == 2);  // a later consumer: another batch size, a new backlog
}

// ---- the walk ----

struct Rng {  // xorshift64*: the same walk on every machine
  uint64_t x;
  uint32_t below(uint32_t n) {
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    return (uint32_t)(((x * 0x2545F4914F6CDD1DULL) >> 33) % n);
  }
};

enum PlaceState { Empty, Acquired, Queued };
enum Holder { Nobody, Producer, Consumer };
struct ModelSlot {
  Holder holder;
  std::vector<PlaceState> places;
  uint64_t openedAt;  // when the producer opened it
};
struct ModelRing {
  bool attached;
  std::vector<ModelSlot> slots;
  int lastUsed;           // the slot opened, or reserved, last; -1 before the first
  int lastSealed;         // the slot a take or a reserve handed the consumer last
  std::deque<int> held;   // the slots the consumer holds, oldest first
};

enum Outcome {
  AcquireGoesOn, AcquireNextRing, AcquireSameRingNewBatch, AcquireNextSlot, AcquireFallThrough, NoneQueueFull, NoneBacklog, NoneInFlight, NoneAllQueued, NoneNoRing,
  QueuedWakes, QueuedSilent, TakeFull, TakePartial, TakeBehindFill, TakeNothing, ReserveFull, ReservePartial, ReserveNothing, DetachedYieldsNothing,
  Released, AttachFirstBacklog, AttachFirstEmpty, AttachAnother, AttachRefused, DetachWithQueued, DetachEmpty, DetachLast, PlainPopOfBacklog, N_OUTCOMES
};
static const char *const kOutcomeNames[N_OUTCOMES] = {
  "acquire: batch goes on", "acquire: next ring's turn", "acquire: same ring, new batch", "acquire: on to the ring's next slot", "acquire: fell through a ring whose next slot is in flight",
  "none: queue full", "none: backlog left", "none: a next slot in flight", "none: every slot full and still queued", "none: no ring", "queued: wakes", "queued: silent", "take: full slot", "take: partial batch sealed",
  "take: a slot behind the fill slot", "take: nothing", "reserve: a slot's worth", "reserve: the rest", "reserve: nothing", "detached ring yields nothing", "release",
  "attach: first, with a backlog", "attach: first, empty queue", "attach: another ring", "attach: refused", "detach: with queued places", "detach: empty", "detach: last ring", "plain pop of the backlog"};
static uint64_t g_outcomes[N_OUTCOMES];

struct Walk {
  StagingRings core;
  std::vector<ModelRing> rings;
  Rng &rng;
  uint32_t cap, bound;
  size_t pooled, backlog;  // pooled messages in the queue; those of them that were there at the first attach
  int current;             // the ring of the last acquire (the first ring attached, before)
  uint64_t clock;

  Walk(Rng &r) : rng(r), cap(1 + r.below(3)), bound(2 + r.below(30)), pooled(r.below(bound + 1)), backlog(0), current(0), clock(0) {}

  uint32_t attached() const {
    uint32_t n = 0;
    for (const ModelRing &g : rings) n += g.attached;
    return n;
  }
  size_t queuedIn(const ModelRing &g) const {
    size_t n = 0;
    for (const ModelSlot &s : g.slots)
      if (s.holder == Producer)
        for (PlaceState p : s.places) n += p == Queued;
    return n;
  }
  size_t queued() const {
    size_t n = 0;
    for (const ModelRing &g : rings)
      if (g.attached) n += queuedIn(g);
    return n;
  }
  static int firstEmpty(const ModelSlot &s) {
    for (size_t i = 0; i < s.places.size(); i++)
      if (s.places[i] == Empty) return (int)i;
    return -1;
  }
  // where a batch may go on or start in g: its last slot while the producer still holds it and it has room; else the next in ring
  // order, if nobody holds that one.  *inFlight: the consumer does.
  int usable(const ModelRing &g, bool *inFlight) const {
    *inFlight = false;
    if (g.lastUsed >= 0 && g.slots[g.lastUsed].holder == Producer && firstEmpty(g.slots[g.lastUsed]) >= 0) return g.lastUsed;
    const int next = (g.lastUsed + 1) % (int)g.slots.size();
    if (g.slots[next].holder == Nobody) return next;
    *inFlight = g.slots[next].holder == Consumer;
    return -1;
  }

  void check() {
    REQUIRE(core.Attached() == attached() && core.Queued() == queued() && core.Unstaged() == backlog && backlog <= pooled);
    for (size_t r = 0; r < rings.size(); r++) {
      REQUIRE(core.IsAttached((int)r) == rings[r].attached);
      if (rings[r].attached) REQUIRE(core.Queued((int)r) == queuedIn(rings[r]));
    }
    REQUIRE(!core.IsAttached(-1) && !core.IsAttached((int)rings.size()));
  }

  void acquire() {
    const bool room = pooled + queued() < bound;
    // the model's answer
    int want = -1, wantSlot = -1;
    bool fellThrough = false;
    const int R = (int)rings.size();
    if (attached() && !backlog && room) {
      if (rings[current].attached && rings[current].lastUsed >= 0) {
        const ModelSlot &s = rings[current].slots[rings[current].lastUsed];
        if (s.holder == Producer && firstEmpty(s) >= 0) want = current, wantSlot = rings[current].lastUsed;  // the batch in progress
      }
      for (int k = 1; want < 0 && k <= R; k++) {
        const int r = (current + k) % R;
        if (!rings[r].attached) continue;
        bool inFlight;
        const int sl = usable(rings[r], &inFlight);
        if (sl >= 0) want = r, wantSlot = sl;
        else if (inFlight) fellThrough = true;
      }
    }
    Place p;
    const bool got = core.Acquire(room, &p);
    REQUIRE(got == (want >= 0));  // "none" exactly when the model finds no attached ring with a usable slot, or the queue is full
    if (!got) {
      g_outcomes[!attached() ? NoneNoRing : backlog ? NoneBacklog : !room ? NoneQueueFull : fellThrough ? NoneInFlight : NoneAllQueued]++;
      check();
      return;
    }
    REQUIRE(backlog == 0);  // no place is acquired while an unstaged message remains
    REQUIRE(p.ring == want && p.slot == wantSlot);
    ModelRing &g = rings[p.ring];
    ModelSlot &s = g.slots[p.slot];
    REQUIRE(g.attached && p.index < cap);
    REQUIRE(s.holder != Consumer && s.places[p.index] == Empty);  // never a place that is queued, or whose slot is in flight
    REQUIRE((int)p.index == firstEmpty(s));                       // a slot fills from place 0 up
    g_outcomes[p.ring != current ? (fellThrough ? AcquireFallThrough : AcquireNextRing) : s.holder == Producer ? AcquireGoesOn : AcquireSameRingNewBatch]++;
    if (s.holder == Nobody) {
      REQUIRE(p.slot == (g.lastUsed + 1) % (int)g.slots.size());  // slots are opened in ring order
      if (g.lastUsed >= 0 && g.slots[g.lastUsed].holder == Producer) g_outcomes[AcquireNextSlot]++;  // (past one that is full and still queued)
      s.holder = Producer;
      s.openedAt = ++clock;
      g.lastUsed = p.slot;
    }
    s.places[p.index] = Acquired;
    current = p.ring;
    // ... and, the samples being in, the place is queued: the queue does both under one hold of its lock
    g_step++;
    const bool wasEmpty = queuedIn(g) == 0;
    REQUIRE(core.MarkQueued(p.ring) == wasEmpty);
    g_outcomes[wasEmpty ? QueuedWakes : QueuedSilent]++;
    s.places[p.index] = Queued;
    check();
  }

  void take(int r) {
    ModelRing &g = rings[r];
    int slot = -1;
    uint32_t n = 0;
    if (!g.attached) {
      REQUIRE(!core.Take(r, &slot, &n) && !core.Reserve(r, &slot, &n));  // a detached ring yields nothing
      g_outcomes[DetachedYieldsNothing]++;
      return check();
    }
    if ((int)g.held.size() >= (int)g.slots.size()) return;  // (the consumer's part: it asks only with a slot to spare)
    if (backlog) {  // the queue asks for these first
      const uint32_t want = backlog < cap ? (uint32_t)backlog : cap;
      REQUIRE(core.Reserve(r, &slot, &n) && n == want);
      REQUIRE(slot == (g.lastSealed + 1) % (int)g.slots.size() && g.slots[slot].holder == Nobody);
      g.slots[slot].holder = Consumer;
      g.lastUsed = g.lastSealed = slot;
      g.held.push_back(slot);
      backlog -= n;
      pooled -= n;
      g_outcomes[n == cap ? ReserveFull : ReservePartial]++;
      return check();
    }
    REQUIRE(!core.Reserve(r, &slot, &n));
    g_outcomes[ReserveNothing]++;
    int oldest = -1;  // the slot the producer opened first among those it still holds
    for (size_t k = 0; k < g.slots.size(); k++)
      if (g.slots[k].holder == Producer && (oldest < 0 || g.slots[k].openedAt < g.slots[oldest].openedAt)) oldest = (int)k;
    if (oldest < 0) {
      REQUIRE(!core.Take(r, &slot, &n));
      g_outcomes[TakeNothing]++;
      return check();
    }
    uint32_t want = 0;
    for (PlaceState p : g.slots[oldest].places) want += p == Queued;
    REQUIRE(want > 0 && core.Take(r, &slot, &n) && slot == oldest && n == want);
    REQUIRE(slot == (g.lastSealed + 1) % (int)g.slots.size());  // within a ring, slots are sealed in ring order
    for (uint32_t i = 0; i < cap; i++) REQUIRE(g.slots[slot].places[i] == (i < n ? Queued : Empty));  // places 0 .. n-1 of it
    g_outcomes[n == cap ? TakeFull : TakePartial]++;
    if (slot != g.lastUsed) g_outcomes[TakeBehindFill]++;
    g.slots[slot].holder = Consumer;
    g.lastSealed = slot;
    g.held.push_back(slot);
    check();
  }

  void release(int r) {
    ModelRing &g = rings[r];
    if (g.held.empty()) return;
    const int slot = g.held.front();  // (the consumer's part: oldest first)
    g.held.pop_front();
    core.Release(r, slot);
    g.slots[slot].holder = Nobody;
    g.slots[slot].places.assign(cap, Empty);
    g_outcomes[Released]++;
    check();
  }

  void attach() {
    const bool refuse = rng.below(4) == 0;
    const uint32_t nSlots = refuse && rng.below(2) ? rng.below(2) : 2 + rng.below(3);
    const uint32_t per = !refuse ? cap : nSlots < 2 ? cap : attached() ? cap + 1 + rng.below(2) : 0;
    const int id = core.Attach(nSlots, per, pooled);
    if (refuse) {
      REQUIRE(id == -1);
      g_outcomes[AttachRefused]++;
      return check();
    }
    REQUIRE(id == (int)rings.size());
    if (!attached()) {
      backlog = pooled;
      current = id;
      g_outcomes[pooled ? AttachFirstBacklog : AttachFirstEmpty]++;
    } else {
      g_outcomes[AttachAnother]++;
    }
    ModelRing g;
    g.attached = true;
    g.slots.assign(nSlots, ModelSlot{Nobody, std::vector<PlaceState>(cap, Empty), 0});
    g.lastUsed = g.lastSealed = -1;
    rings.push_back(g);
    check();
  }

  void detach(int r) {
    ModelRing &g = rings[r];
    const size_t want = g.attached ? queuedIn(g) : 0;
    REQUIRE(core.Detach(r) == want);
    if (g.attached) {
      g.attached = false;
      g_outcomes[want ? DetachWithQueued : DetachEmpty]++;
      if (!attached()) {
        backlog = 0;
        g_outcomes[DetachLast]++;
      }
    }
    check();
  }

  void step() {
    g_step++;
    const uint32_t live = attached(), dice = rng.below(1000);
    if (rings.empty() || (dice < 12 && live < 3) || (!live && dice < 150)) return attach();
    const int r = (int)rng.below((uint32_t)rings.size());
    if (dice < 18) return detach(r);
    if (!live) {  // nobody attached: the producer's appends are pooled messages, a plain consumer pops them
      if (dice < 700 && pooled < bound) pooled++;
      else if (pooled) pooled--;
      Place p;
      REQUIRE(!core.Acquire(true, &p));
      g_outcomes[NoneNoRing]++;
      return check();
    }
    if (dice < 30 && backlog) {  // a consumer without a ring takes one of the backlog the plain way
      core.UnstagedTaken();
      backlog--;
      pooled--;
      g_outcomes[PlainPopOfBacklog]++;
      return check();
    }
    if (dice < 520) return acquire();
    if (dice < 760) return take(r);
    return release(r);
  }
};

int main() {
  scripted();
  Rng rng = {0x5ca1ab1e2024ULL};
  for (int episode = 0; episode < 400; episode++) {  // each a queue of its own: a batch size, a bound, rings that come and go
    Walk w(rng);
    for (int k = 0; k < 1000; k++) w.step();
  }
  bool all = g_step >= 200000;
  for (int k = 0; k < N_OUTCOMES; k++) {
    printf("%10llu  %s\n", (unsigned long long)g_outcomes[k], kOutcomeNames[k]);
    all = all && g_outcomes[k] > 0;
  }
  printf("%llu operations\n", (unsigned long long)g_step);
  if (!all) {
    fprintf(stderr, "FAIL: the walk is too short or left a transition out\n");
    return 1;
  }
  printf("staging rings tests ok\n");
  return 0;
}
