// A slot's life cycle (scanner_amd/csrc/scn_slot_life.h) as a stand-alone program: built by g++ -x c++ together with scn_host.hip, no
// HIP header on the include path, plain and under ASan + UBSan (tests/test_slot_life_cpp.py).
//
// Two slots of one plan, for each kind of plan.  Every state that the transitions reach from two untouched slots is visited once;
// in each, every row of slot_life_table() that applies to the kind is evaluated on slot 0 -- its require_* in the row's order --
// against EXPECT below: one status per entry point and named state, written out from the header's prose.  What state a slot is in
// comes from this program's own record of what has happened to it (Shadow), never from the members of SlotLife; after every
// transition the members are held to that record.
//
//   test_slot_life           prints `slot life tests ok (<states> states, <cells> cells)`
//   test_slot_life --print   prints the expected table, one line `entry_point state status` per cell
#include <cstdio>
#include <cstring>
#include <deque>
#include <set>
#include <string>
#include <tuple>

#include "scn_slot_life.h"

static int g_failed = 0;
static std::string g_where;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    if (!(cond)) {                                                                             \
      std::printf("FAILED %s:%d: %s  (%s)\n", __FILE__, __LINE__, #cond, g_where.c_str());     \
      g_failed++;                                                                              \
    }                                                                                          \
  } while (0)

// the named states of a slot, in the order of EXPECT's columns
enum State { NEVER, PENDING, COLLECTED, EMPTY, NO_LIST, FOLDED, STALE, N_STATES };
static const char *const kStateName[N_STATES] = {"never_submitted", "pending", "collected", "collected_empty", "no_list", "folded", "folded_stale"};
// never_submitted: nothing was ever submitted on the slot.   pending: a submit is queued and not collected.
// collected: free, the list of its last collect still on the device, >= 1 unit.   collected_empty: the same of a submit of 0 units.
// no_list: free, submitted before, no list: a plan without SCN_OUT_HITS, a table change since the collect, a refused collect or a
//   submit that failed half way.   folded: a list that is the history's latest fold.   folded_stale: folded, and the history has
//   moved on (another slot's fold, scn_plan_set_history).
//
// o SCN_OK, S SCN_E_STATE.  Two rules beside the columns: with ANOTHER slot pending, the rows that require no slot pending
// (scn_plan_set_*, scn_plan_update_baseline) are S in every state; with a list of a submit that ran under a floor window,
// scn_collect_floor is SCN_E_INVALID where the column says o.
struct Expect {
  const char *name;
  const char *by_state;  // N_STATES characters
};
static const Expect EXPECT[] = {
    //                             never pending collected empty no_list folded stale
    {"scn_plan_destroy", "ooooooo"},
    {"scn_plan_average_parts", "ooooooo"},
    {"scn_buffer_bytes", "ooooooo"},
    {"scn_host_buffer", "ooooooo"},
    {"scn_submit", "oSooooo"},  // a free slot takes a submit, whatever it holds
    {"scn_submit_device", "oSooooo"},
    {"scn_plan_set_table", "oSooooo"},  // no slot pending
    {"scn_submit_indexed", "oSooooo"},
    {"scn_submit_device_indexed", "oSooooo"},
    {"scn_collect", "SoSSSSS"},  // only a pending submit can be waited for or collected
    {"scn_collect/refused", "SoSSSSS"},
    {"scn_collect_more", "SSooSoo"},  // a list: free, collected with hits, no submit and no table change since
    {"scn_hits_view", "SSooSoo"},
    {"scn_collect_signals", "SSooSoo"},
    {"scn_collect_floor", "SSooSoo"},
    {"scn_plan_set_floor_window", "oSooooo"},
    {"scn_plan_set_baseline", "oSooooo"},
    {"scn_plan_update_baseline", "SSooooo"},  // no slot pending, and a submit to learn from: any accepted one, for good
    {"scn_plan_get_baseline", "ooooooo"},
    {"scn_plan_set_history", "ooooooo"},
    {"scn_plan_update_history", "SSooSSS"},  // a list that has not been folded yet
    {"scn_plan_get_history", "ooooooo"},
    {"scn_collect_confirmed", "SSSSSoS"},  // a list that is the history's latest fold
    {"scn_plan_set_trace", "ooooooo"},
    {"scn_plan_update_trace", "SSooSoo"},  // a list: its spectrum and its centres are what the fold reads (0 units: nothing to fold)
    {"scn_plan_get_trace", "ooooooo"},
    {"scn_plan_merge_trace", "ooooooo"},
    {"scn_plan_trace_emitters", "ooooooo"},
    {"scn_plan_set_levels", "ooooooo"},
    {"scn_plan_update_levels", "SSooSoo"},
    {"scn_plan_get_levels", "ooooooo"},
    {"scn_plan_levels_summary", "ooooooo"},
    {"scn_collect_time_domain", "SoSSSSS"},
    {"scn_convert_raw", "ooooooo"},
    {"scn_wait", "SoSSSSS"},
    {"scn_plan_stream", "ooooooo"},
    {"scn_slot_stream", "ooooooo"},
    {"scn_device_spectrum", "ooooooo"},
    {"scn_plan_window", "ooooooo"},
    {"scn_gather_hits_device", "SSooSoo"},
    {"scn_gather_post", "SSooSoo"},
};
static const size_t N_EXPECT = sizeof(EXPECT) / sizeof(EXPECT[0]);

// the kinds of plan: what a submit's facts are made from, and which rows can be called on it with otherwise valid arguments
enum Kind { SPECTRUM_ONLY, FIXED, FLOOR, BASELINE, TIME_DOMAIN, N_KINDS };
static const char *const kKindName[N_KINDS] = {"spectrum-only", "fixed", "floor", "baseline", "time-domain"};
static bool kind_hits(int k) { return k == FIXED || k == FLOOR || k == BASELINE; }
static bool applies(const char *name, int k) {
  const auto is = [&](const char *n) { return !std::strcmp(name, n); };
  if (is("scn_collect_time_domain")) return k == TIME_DOMAIN;
  if (is("scn_collect") || is("scn_collect/refused")) return k != TIME_DOMAIN;
  if (is("scn_collect_floor") || is("scn_plan_set_floor_window")) return k == FLOOR;
  if (is("scn_plan_set_baseline") || is("scn_plan_update_baseline") || is("scn_plan_get_baseline")) return k == BASELINE;
  if (is("scn_collect_more") || is("scn_hits_view") || is("scn_collect_signals") || is("scn_gather_hits_device") || is("scn_gather_post") ||
      is("scn_plan_set_history") || is("scn_plan_update_history") || is("scn_plan_get_history") || is("scn_collect_confirmed"))
    return kind_hits(k);
  // (a trace or a level histogram: a plan with hits whose submits store a spectrum -- a fixed plan with SCN_OUT_SPECTRUM beside its hits)
  if (!std::strncmp(name, "scn_plan_", 9) && (std::strstr(name, "_trace") || std::strstr(name, "_levels"))) return kind_hits(k);
  return true;
}

// what has happened to a slot, recorded by this program
struct Shadow {
  bool submitted = false, pending = false, list = false, built = false, windowed = false;
  int fold = 0;  // 0: not folded, 1: the latest fold, 2: folded, the history has moved on
  uint32_t units = 0, total = 0;
};
static State state_of(const Shadow &s) {
  if (s.pending) return PENDING;
  if (!s.submitted) return NEVER;
  if (!s.list) return NO_LIST;
  if (s.fold) return s.fold == 1 ? FOLDED : STALE;
  return s.units ? COLLECTED : EMPTY;
}

struct World {
  SlotLife life[2];
  Shadow sh[2];
  uint64_t epoch = 0;
};
static const uint32_t kHistoryRows = 2;

static int status_of(char c) { return c == 'o' ? SCN_OK : c == 'S' ? SCN_E_STATE : SCN_E_INVALID; }
static const char *status_name(int st) { return st == SCN_OK ? "SCN_OK" : st == SCN_E_STATE ? "SCN_E_STATE" : "SCN_E_INVALID"; }
static bool needs_none_pending(const char *name) {
  return !std::strcmp(name, "scn_plan_set_table") || !std::strcmp(name, "scn_plan_set_floor_window") || !std::strcmp(name, "scn_plan_set_baseline") ||
         !std::strcmp(name, "scn_plan_update_baseline");
}
static int expected(const Expect &e, const World &w) {
  if (w.sh[1].pending && needs_none_pending(e.name)) return SCN_E_STATE;
  const int st = status_of(e.by_state[state_of(w.sh[0])]);
  if (st == SCN_OK && !std::strcmp(e.name, "scn_collect_floor") && w.sh[0].windowed) return SCN_E_INVALID;
  return st;
}

// a row's requirements on slot 0, in the row's order: the first status that is not SCN_OK
static int evaluate(const SlotLifeRow &row, const World &w) {
  const SlotLife *const lives[2] = {&w.life[0], &w.life[1]};
  for (const SlotRequirement &r : row.require) {
    int st = SCN_OK;
    switch (r.req) {
      case SlotReq::None: break;
      case SlotReq::Free: st = require_free(w.life[0], 0); break;
      case SlotReq::Pending: st = require_pending(w.life[0], 0); break;
      case SlotReq::List: st = require_list(w.life[0], 0, r.text); break;
      case SlotReq::NonePending: st = require_none_pending(lives, 2, r.text); break;
      case SlotReq::Unfolded: st = require_unfolded(w.life[0], 0); break;
      case SlotReq::LatestFold: st = require_latest_fold(w.life[0], 0, w.epoch, kHistoryRows); break;
      case SlotReq::Learnable: st = require_learnable(w.life[0], 0); break;
      case SlotReq::UnitFloor: st = require_unit_floor(w.life[0], 0); break;
    }
    if (st) return st;
  }
  return SCN_OK;
}

// the members against the record
static void hold(const World &w, int kind) {
  for (int i = 0; i < 2; i++) {
    const SlotLife &l = w.life[i];
    const Shadow &s = w.sh[i];
    CHECK(l.pending == s.pending);
    CHECK(l.list_valid == s.list);
    CHECK(l.list_built == s.built);
    CHECK(l.floor_windowed == s.windowed);
    CHECK(l.base_submitted == (s.submitted && kind == BASELINE));
    CHECK((l.folded_epoch != 0) == (s.fold != 0));
    CHECK(!s.fold || (l.folded_epoch == w.epoch) == (s.fold == 1));
    CHECK(l.n_buffers == s.units);
    CHECK(l.total_hits == s.total);
  }
}

static void history_moves_on(World &w) {
  w.epoch++;
  for (Shadow &s : w.sh)
    if (s.fold == 1) s.fold = 2;
}

// -- the transitions, each applied to the members through the header and to the record by hand -------------------------------------
// queued: everything was queued (else: a HIP call failed half way, after on_submit); eager: the list was built behind the launch
static void submit(World &w, int i, int kind, uint32_t units, bool windowed, bool queued, bool eager) {
  const SubmitFacts f = {units, kind_hits(kind), windowed, kind == BASELINE, kind == TIME_DOMAIN};
  const bool flips = on_submit(w.life[i], f);
  CHECK(flips == submit_flips(f));
  CHECK(flips == (kind_hits(kind) && units != 0));  // the other generation exactly when there are hits to write
  Shadow &s = w.sh[i];
  s.submitted = true;
  s.units = units;
  if (kind != TIME_DOMAIN) {  // (a time-domain submit has units and nothing else)
    s.list = s.built = false;
    s.windowed = windowed;
  }
  if (eager && flips) {
    on_list_built(w.life[i]);
    s.built = true;
  }
  if (queued) {
    on_submitted(w.life[i]);
    s.pending = true;
  }
}
static void take(World &w, int i) {
  on_take(w.life[i]);
  w.sh[i].pending = false;
}
static void collect(World &w, int i, int kind, bool too_many) {
  take(w, i);
  Shadow &s = w.sh[i];
  const uint64_t total = too_many ? 0x80000000ull : kind_hits(kind) && s.units ? 5u : 0u;
  const int st = on_collect(w.life[i], kind_hits(kind), total);
  CHECK(st == (too_many ? SCN_E_INVALID : SCN_OK));
  s.list = kind_hits(kind);
  s.fold = 0;
  if (!too_many) s.total = (uint32_t)total;  // (refused: the total stays the last collect's)
}

typedef std::tuple<bool, bool, bool, bool, bool, int, uint32_t, uint32_t> SlotKey;
static SlotKey key_of(const SlotLife &l, uint64_t epoch) {
  return SlotKey(l.pending, l.list_valid, l.list_built, l.floor_windowed, l.base_submitted, !l.folded_epoch ? 0 : l.folded_epoch == epoch ? 1 : 2,
                 l.n_buffers, l.total_hits);
}

static void print_table() {
  for (const Expect &e : EXPECT) {
    for (int s = 0; s < N_STATES; s++) std::printf("%s %s %s\n", e.name, kStateName[s], status_name(status_of(e.by_state[s])));
    if (needs_none_pending(e.name)) std::printf("%s other_slot_pending SCN_E_STATE\n", e.name);
    if (!std::strcmp(e.name, "scn_collect_floor")) std::printf("%s collected_windowed SCN_E_INVALID\n", e.name);
  }
}

static void check_messages() {
  SlotLife l, other;
  const SlotLife *const lives[2] = {&other, &l};
  const auto said = [](const char *text) { return !std::strcmp(scn_last_error(), text); };
  g_where = "messages";
  l.pending = true;
  CHECK(require_free(l, 3) == SCN_E_STATE && said("slot 3 has an uncollected submit"));
  CHECK(require_none_pending(lives, 2, "") == SCN_E_STATE && said("slot 1 has an uncollected submit"));
  CHECK(require_none_pending(lives, 2, ": its records still read the table") == SCN_E_STATE &&
        said("slot 1 has an uncollected submit: its records still read the table"));
  CHECK(require_none_pending(lives, 2, ": its detect kernel may still read the baseline") == SCN_E_STATE &&
        said("slot 1 has an uncollected submit: its detect kernel may still read the baseline"));
  l.pending = false;
  CHECK(require_pending(l, 2) == SCN_E_STATE && said("slot 2 has nothing submitted"));
  CHECK(require_list(l, 1, "hit list is still on the device") == SCN_E_STATE && said("slot 1: no collected submit whose hit list is still on the device"));
  CHECK(require_list(l, 1, "hit list is still available") == SCN_E_STATE && said("slot 1: no collected submit whose hit list is still available"));
  CHECK(require_list(l, 1, "floor is still available") == SCN_E_STATE && said("slot 1: no collected submit whose floor is still available"));
  CHECK(require_learnable(l, 0) == SCN_E_STATE && said("slot 0 has no collected submit to learn from"));
  CHECK(require_latest_fold(l, 2, 0, 1) == SCN_E_STATE && said("slot 2: its submit is not the history's latest fold (scn_plan_update_history)"));
  l.folded_epoch = 7;
  CHECK(require_latest_fold(l, 2, 7, 0) == SCN_E_STATE);  // (the history was dropped)
  CHECK(require_latest_fold(l, 2, 7, 1) == SCN_OK);
  CHECK(require_unfolded(l, 3) == SCN_E_STATE && said("slot 3: its submit is already part of the history"));
  l.floor_windowed = true;
  CHECK(require_unit_floor(l, 1) == SCN_E_INVALID &&
        said("slot 1 was submitted under a floor window: every bin has a floor of its own (scn_local_floor_from_spectrum), no unit has one"));
  CHECK(on_collect(l, true, 0x80000000ull) == SCN_E_INVALID && said("2147483648 hits in one submit: split the batch"));
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--print")) {
    print_table();
    return 0;
  }
  size_t n_rows = 0;
  const SlotLifeRow *rows = slot_life_table(&n_rows);
  g_where = "the table's rows";
  CHECK(n_rows == N_EXPECT);
  for (size_t r = 0; r < n_rows && r < N_EXPECT; r++) CHECK(!std::strcmp(rows[r].name, EXPECT[r].name) && std::strlen(EXPECT[r].by_state) == N_STATES);
  check_messages();
  if (g_failed) return 1;

  unsigned states = 0, cells = 0;
  bool seen_state[N_KINDS][N_STATES] = {};
  for (int kind = 0; kind < N_KINDS; kind++) {
    std::set<std::tuple<SlotKey, SlotKey>> seen;
    std::deque<World> todo;
    const auto visit = [&](const World &w) {
      hold(w, kind);
      if (seen.insert(std::make_tuple(key_of(w.life[0], w.epoch), key_of(w.life[1], w.epoch))).second) todo.push_back(w);
    };
    visit(World());
    while (!todo.empty()) {
      const World w = todo.front();
      todo.pop_front();
      states++;
      seen_state[kind][state_of(w.sh[0])] = true;
      for (size_t r = 0; r < n_rows; r++) {
        if (!applies(rows[r].name, kind)) continue;
        g_where = std::string(kKindName[kind]) + " plan, " + rows[r].name + " in " + kStateName[state_of(w.sh[0])] + (w.sh[1].pending ? ", the other slot pending" : "") +
                  (w.sh[0].windowed ? ", windowed" : "");
        const int st = evaluate(rows[r], w);
        cells++;
        CHECK(st == expected(EXPECT[r], w));
        if (st != SCN_OK) continue;
        // an accepted call moves the slot as its row says
        World next = w;
        switch (rows[r].move) {
          case SlotMove::None: break;
          case SlotMove::Submit:
            for (uint32_t units = 0; units < 6; units += 3)
              for (int windowed = 0; windowed < (kind == FLOOR ? 2 : 1); windowed++)
                for (int how = 0; how < 3; how++) {  // queued; queued with the list built behind the launch; failed half way
                  next = w;
                  submit(next, 0, kind, units, windowed != 0, how < 2, how == 1);
                  visit(next);
                }
            break;
          case SlotMove::Collect:
            for (int too_many = 0; too_many < (kind_hits(kind) && w.sh[0].units ? 2 : 1); too_many++) {
              next = w;
              collect(next, 0, kind, too_many != 0);
              visit(next);
            }
            break;
          case SlotMove::Take:
          case SlotMove::CollectTimeDomain:
            if (rows[r].move == SlotMove::Take) take(next, 0);
            else {
              on_collect_time_domain(next.life[0]);
              next.sh[0].pending = false;
            }
            visit(next);
            break;
          case SlotMove::TableChange: {
            SlotLife *const lives[2] = {&next.life[0], &next.life[1]};
            on_table_change(lives, 2);
            next.sh[0].list = next.sh[1].list = false;
            visit(next);
            break;
          }
          case SlotMove::Fold:
            history_moves_on(next);
            on_fold(next.life[0], next.epoch);
            next.sh[0].fold = 1;
            visit(next);
            break;
          case SlotMove::EpochAdvance:
            history_moves_on(next);
            visit(next);
            break;
        }
      }
      // a list that holds records is built on demand by whoever reads it first
      if (state_of(w.sh[0]) != PENDING && w.sh[0].list && w.sh[0].total && !w.sh[0].built) {
        World next = w;
        on_list_built(next.life[0]);
        next.sh[0].built = true;
        visit(next);
      }
      // the other slot: submitted, collected
      g_where = std::string(kKindName[kind]) + " plan, the other slot";
      World next = w;
      if (!w.sh[1].pending) submit(next, 1, kind, 3, false, true, false);
      else if (kind == TIME_DOMAIN) {
        on_collect_time_domain(next.life[1]);
        next.sh[1].pending = false;
      } else collect(next, 1, kind, false);
      visit(next);
    }
  }
  // every named state was met on a plan that can hold it
  g_where = "states met";
  for (int kind = 0; kind < N_KINDS; kind++)
    for (int s = 0; s < N_STATES; s++) CHECK(seen_state[kind][s] == (s <= PENDING || s == NO_LIST || kind_hits(kind)));
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("slot life tests ok (%u states, %u cells)\n", states, cells);
  return 0;
}
