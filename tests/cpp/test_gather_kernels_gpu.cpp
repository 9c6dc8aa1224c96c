// test_gather_kernels_gpu.cpp -- the steady-state gather's two kernels (scanner_amd/csrc/scn_gather_kernels.h) on ONE GPU at
// world sizes 1, 2, 3 and 8.  The compaction kernel reads a ring in device memory; this program fills that ring with what
// `world` ranks would have sent and holds everything the kernels write, byte for byte, to a host model:
//   * the rank acting as the root is packed straight into its ring slot (as scn_gather_post does), every other rank into an
//     outgoing buffer of its own, which a device-to-device hipMemcpyAsync moves into the ring (it stands in for the send /
//     receive pair); pack launches, copies and the compaction run back to back on one non-blocking stream, one event
//     synchronisation at the end;
//   * grids and addresses are the production ones: scn_launch_gather_pack / scn_launch_gather_compact, scn_gather_ring_at,
//     scn_gather_out_at, scn_gather_list_at, scn_gather_heads_at;
//   * the model: scn_stream_outcome over the headers as they stand in the ring is the DEFINITION of the list -- for each rank,
//     in order, the first offsets[r + 1] - offsets[r] records of its message at offsets[r].  The intact predicate is not restated.
//   * the list and the headers live in hipHostMalloc memory, sized exactly and pre-filled with 0xA5; the ring and the outgoing
//     buffers are device memory, sized exactly, pre-filled with 0xA5 and compared whole against host mirrors afterwards.
// One line per case on stdout: `case <name> ok ...` or `case <name> FAIL <what>`.  Exit 1 on any mismatch; exit 3 at once on
// any HIP error (nothing further is launched).  `--only <substring>` runs the sessions with a case of that name.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scn_gather_kernels.h"
#include "scn_gather_protocol.h"

namespace {
const char *g_where = "(start)";
int g_failed = 0, g_cases = 0;
const char *g_only = nullptr;
uint32_t g_post_no = 0;  // the "case" the record contents are a function of

[[noreturn]] void hip_fatal(const char *call, hipError_t e, int line) {
  printf("hip-error case=%s line=%d %s: %s\n", g_where, line, call, hipGetErrorString(e));
  fflush(stdout);
  _Exit(3);  // nothing further is launched, nothing is torn down through the runtime
}
#define HIP(call)                                        \
  do {                                                   \
    hipError_t e_ = (call);                              \
    if (e_ != hipSuccess) hip_fatal(#call, e_, __LINE__); \
  } while (0)

[[noreturn]] void program_bug(const char *what) {
  printf("program-bug case=%s %s\n", g_where, what);
  fflush(stdout);
  _Exit(4);
}

const size_t REC = sizeof(scn_hit);
const uint8_t FILL = 0xA5;
static_assert(sizeof(scn_hit) == 24, "three 8-byte words");

// all 24 bytes of a record are a function of (rank, index, case): a misplaced 8-byte word shows
scn_hit record(uint32_t post, uint32_t rank, uint32_t k) {
  static const uint32_t special[] = {0x7fc00001u, 0xffc12345u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fa00bb1u, 0x00000001u, 0xc2c80000u};
  scn_hit h;
  h.seq_id = ((uint64_t)(post + 1u) << 32) + ((uint64_t)rank << 24) + k;                  // above 2^32
  h.i = (k & 1u) ? (uint32_t)(-(int32_t)(k + 1u + rank)) : k + 7u * rank;                 // negative and positive as int32
  const uint32_t bits = (k % 3u == 0u) ? special[(k / 3u + rank) % 8u] : 0x41200000u + 977u * k + 31u * rank + post;  // NaN payloads, -0.0, infinities, ...
  memcpy(&h.power_db, &bits, 4);
  h.freq_hz = 0x9E3779B97F4A7C15ull * ((((uint64_t)post * 8u + rank) << 20) + k + 1u);    // distinct: an odd multiplier is a bijection
  return h;
}

struct RankSpec {
  ScnStreamHeader pack;        // what the pack kernel is given: pack.sent <= n_src <= cap always (the launch stays in bounds)
  uint32_t n_src = 0;          // records of the rank's source list (0: a null source)
  bool rewrite = false;        // the header in the ring is overwritten after arrival (a corruption the pack kernel cannot be asked for)
  ScnStreamHeader ring_head;
  bool arrives = true;         // a peer whose message never reaches the ring: the slot keeps what it held
  uint32_t direct_grid = 0;    // > 0: the pack kernel launched with this grid, not through scn_launch_gather_pack
  uint32_t contributes = 0;    // records of this rank in the list, stated by the case (the model must agree)
};

struct Post {
  std::string name;
  uint64_t seq = 0;
  uint32_t root = 0;
  std::vector<RankSpec> ranks;
  int want_status = SCN_OK;
  int want_bad = -1;
  int count_rank = -1;         // >= 0: outcome.counts[count_rank] must be want_count
  uint32_t want_count = 0;
  // filled in while running
  uint32_t no = 0, tk = 0;
  std::vector<std::vector<scn_hit>> src;
  std::vector<scn_hit *> d_src;
  std::vector<uint8_t> want_list, want_heads;
  ScnGatherOutcome outcome;
};

std::string first_diff(const uint8_t *got, const uint8_t *want, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (got[k] != want[k]) {
      char b[96];
      snprintf(b, sizeof b, "byte %zu (record %zu word %zu) got %02x want %02x", k, k / REC, (k % REC) / 8, got[k], want[k]);
      return b;
    }
  return "";
}

struct Session {
  uint32_t world, cap, tickets;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  scn_hit *d_ring = nullptr;
  std::vector<scn_hit *> d_out;
  scn_hit *h_list = nullptr;
  ScnStreamHeader *h_heads = nullptr, *h_rewrite = nullptr;  // pinned
  std::vector<uint8_t> ring_m;                // host mirrors of the device buffers
  std::vector<std::vector<uint8_t>> out_m;
  size_t ring_n, out_n, list_n, heads_n;      // records

  Session(uint32_t world_, uint32_t cap_, uint32_t tickets_) : world(world_), cap(cap_), tickets(tickets_) {
    ring_n = scn_gather_ring_at(tickets, world, 0, cap);
    out_n = scn_gather_out_at(tickets, cap);
    list_n = scn_gather_list_at(tickets, world, cap);
    heads_n = scn_gather_heads_at(tickets, world);
    HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HIP(hipMalloc(&d_ring, ring_n * REC));
    HIP(hipMemset(d_ring, FILL, ring_n * REC));
    ring_m.assign(ring_n * REC, FILL);
    d_out.assign(world, nullptr);
    out_m.assign(world, std::vector<uint8_t>(out_n * REC, FILL));
    for (uint32_t r = 0; r < world; r++) {
      HIP(hipMalloc(&d_out[r], out_n * REC));
      HIP(hipMemset(d_out[r], FILL, out_n * REC));
    }
    HIP(hipHostMalloc(&h_list, list_n * REC, hipHostMallocDefault));
    HIP(hipHostMalloc(&h_heads, heads_n * REC, hipHostMallocDefault));
    HIP(hipHostMalloc(&h_rewrite, heads_n * REC, hipHostMallocDefault));
    HIP(hipDeviceSynchronize());
  }
  ~Session() {
    HIP(hipDeviceSynchronize());
    for (scn_hit *p : d_out) HIP(hipFree(p));
    HIP(hipFree(d_ring));
    HIP(hipHostFree(h_list));
    HIP(hipHostFree(h_heads));
    HIP(hipHostFree(h_rewrite));
    HIP(hipEventDestroy(done));
    HIP(hipStreamDestroy(stream));
  }

  static void mirror_pack(uint8_t *msg, const ScnStreamHeader &h, const std::vector<scn_hit> &src) {
    memcpy(msg, &h, REC);
    if (h.sent) memcpy(msg + REC, src.data(), (size_t)h.sent * REC);
  }

  // every post of `posts` is enqueued before the first is checked
  void run(std::vector<Post> &posts) {
    bool wanted = !g_only;
    for (const Post &p : posts) wanted = wanted || p.name.find(g_only) != std::string::npos;
    if (!wanted) return;
    memset(h_list, FILL, list_n * REC);
    memset(h_heads, FILL, heads_n * REC);
    std::vector<uint8_t> list_all(list_n * REC, FILL), heads_all(heads_n * REC, FILL);
    // (1) the sources, uploaded before anything is launched
    for (Post &p : posts) {
      g_where = p.name.c_str();
      p.no = g_post_no++;
      p.tk = (uint32_t)(p.seq % SCN_GATHER_TICKETS);
      if (p.ranks.size() != world || p.root >= world || p.tk >= tickets) program_bug("a post that does not fit its session");
      p.src.assign(world, {});
      p.d_src.assign(world, nullptr);
      for (uint32_t r = 0; r < world; r++) {
        const RankSpec &s = p.ranks[r];
        if (s.pack.sent > s.n_src || s.n_src > cap) program_bug("a pack launch that would leave its buffers");
        for (uint32_t k = 0; k < s.n_src; k++) p.src[r].push_back(record(p.no, r, k));
        if (s.n_src) {
          HIP(hipMalloc(&p.d_src[r], (size_t)s.n_src * REC));
          HIP(hipMemcpy(p.d_src[r], p.src[r].data(), (size_t)s.n_src * REC, hipMemcpyHostToDevice));
        }
        if (s.rewrite) h_rewrite[scn_gather_heads_at(p.tk, world) + r] = s.ring_head;
      }
    }
    HIP(hipDeviceSynchronize());
    // (2) pack -> (copy) -> compaction, post after post, no host synchronisation
    for (Post &p : posts) {
      g_where = p.name.c_str();
      for (uint32_t r = 0; r < world; r++) {
        const RankSpec &s = p.ranks[r];
        const size_t in_ring = scn_gather_ring_at(p.tk, world, r, cap), in_out = scn_gather_out_at(p.tk, cap);
        const bool straight = r == p.root;
        scn_hit *msg = straight ? d_ring + in_ring : d_out[r] + in_out;
        if (s.direct_grid) {
          hipLaunchKernelGGL(scn_gather_pack_kernel, dim3(s.direct_grid), dim3(256), 0, stream, (const scn_hit *)p.d_src[r], s.pack, msg);
          HIP(hipGetLastError());
        } else {
          HIP(scn_launch_gather_pack(p.d_src[r], s.pack, msg, stream));
        }
        mirror_pack(straight ? ring_m.data() + in_ring * REC : out_m[r].data() + in_out * REC, s.pack, p.src[r]);
        if (!straight && s.arrives) {
          HIP(hipMemcpyAsync(d_ring + in_ring, d_out[r] + in_out, scn_gather_msg_records(cap) * REC, hipMemcpyDeviceToDevice, stream));
          memcpy(ring_m.data() + in_ring * REC, out_m[r].data() + in_out * REC, scn_gather_msg_records(cap) * REC);
        }
        if (s.rewrite) {
          HIP(hipMemcpyAsync(d_ring + in_ring, h_rewrite + scn_gather_heads_at(p.tk, world) + r, REC, hipMemcpyHostToDevice, stream));
          memcpy(ring_m.data() + in_ring * REC, &s.ring_head, REC);
        }
      }
      const size_t ring0 = scn_gather_ring_at(p.tk, world, 0, cap), list0 = scn_gather_list_at(p.tk, world, cap), heads0 = scn_gather_heads_at(p.tk, world);
      HIP(scn_launch_gather_compact(d_ring + ring0, world, cap, p.seq, h_list + list0, h_heads + heads0, stream));
      // the model, from the headers as they stand in the ring now
      std::vector<ScnStreamHeader> heads(world);
      for (uint32_t r = 0; r < world; r++) memcpy(&heads[r], ring_m.data() + scn_gather_ring_at(p.tk, world, r, cap) * REC, REC);
      p.outcome = scn_stream_outcome(heads.data(), world, cap, p.seq);
      p.want_list.assign((size_t)world * cap * REC, FILL);
      for (uint32_t r = 0; r < world; r++) {
        const uint64_t n = p.outcome.offsets[r + 1] - p.outcome.offsets[r];
        if (p.outcome.offsets[r] + n > (uint64_t)world * cap || n > cap) program_bug("the model leaves the list");
        memcpy(p.want_list.data() + p.outcome.offsets[r] * REC, ring_m.data() + (scn_gather_ring_at(p.tk, world, r, cap) + 1u) * REC, n * REC);
      }
      p.want_heads.assign((const uint8_t *)heads.data(), (const uint8_t *)heads.data() + world * REC);
      memcpy(list_all.data() + list0 * REC, p.want_list.data(), p.want_list.size());
      memcpy(heads_all.data() + heads0 * REC, p.want_heads.data(), p.want_heads.size());
    }
    g_where = posts.back().name.c_str();
    HIP(hipEventRecord(done, stream));
    HIP(hipEventSynchronize(done));
    // (3) the checks
    std::vector<uint8_t> ring_got(ring_n * REC), out_got(out_n * REC);
    HIP(hipMemcpy(ring_got.data(), d_ring, ring_n * REC, hipMemcpyDeviceToHost));
    std::vector<std::vector<uint8_t>> outs_got(world);
    for (uint32_t r = 0; r < world; r++) {
      HIP(hipMemcpy(out_got.data(), d_out[r], out_n * REC, hipMemcpyDeviceToHost));
      outs_got[r] = out_got;
    }
    for (size_t pi = 0; pi < posts.size(); pi++) {
      Post &p = posts[pi];
      g_where = p.name.c_str();
      std::string why;
      auto fail = [&](const std::string &what, const std::string &detail) {
        if (why.empty()) why = what + ": " + detail;
      };
      const size_t list0 = scn_gather_list_at(p.tk, world, cap) * REC, heads0 = scn_gather_heads_at(p.tk, world) * REC;
      const uint64_t total = p.outcome.total;
      const uint8_t *got_list = (const uint8_t *)h_list + list0;
      std::string d = first_diff(got_list, p.want_list.data(), total * REC);
      if (!d.empty()) fail("list[0:total]", d);
      d = first_diff(got_list + total * REC, p.want_list.data() + total * REC, p.want_list.size() - total * REC);
      if (!d.empty()) fail("list[total:world*cap] lost its fill", d);
      d = first_diff((const uint8_t *)h_heads + heads0, p.want_heads.data(), p.want_heads.size());
      if (!d.empty()) fail("heads", d);
      for (uint32_t r = 0; r < world; r++) {
        const RankSpec &s = p.ranks[r];
        const size_t in_ring = scn_gather_ring_at(p.tk, world, r, cap) * REC, in_out = scn_gather_out_at(p.tk, cap) * REC, len = scn_gather_msg_records(cap) * REC;
        char tag[48];
        // the message as the pack kernel had to leave it (header, `sent` records, the fill behind them) and the ring unchanged by the compaction
        snprintf(tag, sizeof tag, "ring message of rank %u", r);
        d = first_diff(ring_got.data() + in_ring, ring_m.data() + in_ring, len);
        if (!d.empty()) fail(tag, d);
        snprintf(tag, sizeof tag, "outgoing message of rank %u", r);
        d = first_diff(outs_got[r].data() + in_out, out_m[r].data() + in_out, len);
        if (!d.empty()) fail(tag, d);
        if (s.n_src) {
          std::vector<uint8_t> back((size_t)s.n_src * REC);
          HIP(hipMemcpy(back.data(), p.d_src[r], back.size(), hipMemcpyDeviceToHost));
          snprintf(tag, sizeof tag, "source of rank %u changed", r);
          d = first_diff(back.data(), (const uint8_t *)p.src[r].data(), back.size());
          if (!d.empty()) fail(tag, d);
        }
      }
      // what the case itself states, beside the model
      uint64_t want_total = 0;
      for (const RankSpec &s : p.ranks) want_total += s.contributes;
      char b[160];
      if (total != want_total) {
        snprintf(b, sizeof b, "scn_stream_outcome counts %llu records, the case states %llu", (unsigned long long)total, (unsigned long long)want_total);
        fail("total", b);
      }
      if (p.outcome.status != p.want_status || p.outcome.bad_rank != p.want_bad) {
        snprintf(b, sizeof b, "status %d bad_rank %d, the case states %d / %d", p.outcome.status, p.outcome.bad_rank, p.want_status, p.want_bad);
        fail("outcome", b);
      }
      if (p.count_rank >= 0 && p.outcome.counts[p.count_rank] != p.want_count) {
        snprintf(b, sizeof b, "counts[%d] = %u, the case states %u", p.count_rank, p.outcome.counts[p.count_rank], p.want_count);
        fail("counts", b);
      }
      if (pi + 1 == posts.size()) {  // ... and nothing anywhere else in the four buffers (other tickets' places included)
        d = first_diff((const uint8_t *)h_list, list_all.data(), list_all.size());
        if (!d.empty()) fail("pinned lists, whole", d);
        d = first_diff((const uint8_t *)h_heads, heads_all.data(), heads_all.size());
        if (!d.empty()) fail("pinned headers, whole", d);
        d = first_diff(ring_got.data(), ring_m.data(), ring_m.size());
        if (!d.empty()) fail("ring, whole", d);
        for (uint32_t r = 0; r < world; r++) {
          d = first_diff(outs_got[r].data(), out_m[r].data(), out_m[r].size());
          if (!d.empty()) fail("outgoing buffer, whole", d);
        }
      }
      g_cases++;
      if (why.empty()) {
        printf("case %s ok world=%u cap=%u root=%u ticket=%u total=%llu status=%d\n", p.name.c_str(), world, cap, p.root, p.tk, (unsigned long long)total, p.outcome.status);
      } else {
        g_failed++;
        printf("case %s FAIL %s\n", p.name.c_str(), why.c_str());
      }
      for (scn_hit *s : p.d_src)
        if (s) HIP(hipFree(s));
    }
    fflush(stdout);
  }
};

// ---- building cases -----------------------------------------------------------------------------------------------------------
RankSpec good(uint64_t seq, uint32_t sent) {
  RankSpec s;
  s.pack = ScnStreamHeader{sent, (uint32_t)SCN_OK, sent, SCN_STREAM_MAGIC, seq};
  s.n_src = s.contributes = sent;
  return s;
}

Post post_of(const std::string &name, uint64_t seq, uint32_t root, const std::vector<uint32_t> &sent) {
  Post p;
  p.name = name;
  p.seq = seq;
  p.root = root;
  for (uint32_t n : sent) p.ranks.push_back(good(seq, n));
  return p;
}

void run_one(uint32_t world, uint32_t cap, Post p) {
  if (g_only && p.name.find(g_only) == std::string::npos) return;
  std::vector<Post> posts{p};
  Session s(world, cap, (uint32_t)(p.seq % SCN_GATHER_TICKETS) + 1u);
  s.run(posts);
}

std::string nm(const char *fmt, ...) {
  char b[128];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  return b;
}

uint32_t root_at(uint32_t world, int where) { return where == 0 ? 0u : where == 1 ? world / 2u : world - 1u; }  // first, middle, last
const char *WHERE[] = {"first", "middle", "last"};
const uint64_t SEQ0 = 0x100000000ull + 40u;  // above 2^32: a comparison of the low word alone shows

std::vector<uint32_t> pattern(int kind, uint32_t world, uint32_t cap) {
  std::vector<uint32_t> v(world, 0u);
  const uint32_t mix[8] = {cap, 0u, 1u, cap - 1u, 0u, 0u, 257u, cap};
  for (uint32_t r = 0; r < world; r++) switch (kind) {
      case 0: v[r] = cap; break;                                  // all cap
      case 1: v[r] = 0u; break;                                   // all 0
      case 2: v[r] = r == 0u ? cap : 0u; break;                   // only the first
      case 3: v[r] = r == world - 1u ? cap : 0u; break;           // only the last
      case 4: v[r] = (r % 3u == 0u || r == world - 1u) ? cap : 0u; break;  // zeros between full ranks
      default: v[r] = mix[world == 8u ? r : (r * 3u + 3u) % 8u] < cap ? mix[world == 8u ? r : (r * 3u + 3u) % 8u] : cap; break;  // a mix (world 3: cap-1, 257, 0 ...)
    }
  return v;
}
const char *PATTERN[] = {"allcap", "allzero", "firstonly", "lastonly", "zerosbetween", "mix"};

void cases_cap_edges() {
  int k = 0;
  for (uint32_t cap : {1u, 85u, 86u, 682u, 683u, 10922u, 10923u, 11000u})
    for (uint32_t world : {1u, 2u, 3u, 8u})
      for (int kind : {0, 5}) {
        const uint32_t root = root_at(world, k % 3);
        run_one(world, cap, post_of(nm("cap_%u_w%u_%s_root%u", cap, world, PATTERN[kind], root), SEQ0 + (uint64_t)(k % 4), root, pattern(kind, world, cap)));
        k++;
      }
}

void cases_sent_edges() {
  const uint32_t cap = 11000u;
  for (uint32_t sent : {0u, 1u, 85u, 86u, 5461u, 5462u, 11000u}) {
    run_one(1, cap, post_of(nm("sent_%u_w1", sent), SEQ0, 0, {sent}));
    for (uint32_t root : {0u, 1u}) run_one(2, cap, post_of(nm("sent_%u_w2_root%u", sent, root), SEQ0 + 1u + root, root, {sent, cap}));
    run_one(3, cap, post_of(nm("sent_%u_w3_last_root1", sent), SEQ0 + 3u, 1, {cap - 1u, 3u, sent}));
  }
}

// the pack kernel's own contract: it strides by its grid, whatever grid it is given (scn_launch_gather_pack never asks for fewer
// workgroups than one pass needs below its cap of 64, so only a direct launch can tell a stride of gridDim.x * 256 from a constant)
void cases_pack_grid() {
  for (uint32_t grid : {1u, 3u, 64u, 65u})
    for (uint32_t sent : {86u, 5462u}) {
      Post p = post_of(nm("packgrid_%u_sent%u", grid, sent), SEQ0, 1, {sent, sent});
      p.ranks[0].direct_grid = p.ranks[1].direct_grid = grid;
      run_one(2, 5462u, p);
    }
}

void cases_patterns() {
  for (uint32_t world : {8u, 3u})
    for (int kind = 0; kind < 6; kind++) {
      for (int where = 0; where < 3; where++)
        run_one(world, 300u, post_of(nm("pattern_w%u_%s_root%s", world, PATTERN[kind], WHERE[where]), SEQ0 + (uint64_t)where, root_at(world, where), pattern(kind, world, 300u)));
      run_one(world, 1u, post_of(nm("pattern_w%u_%s_cap1", world, PATTERN[kind]), SEQ0 + 3u, root_at(world, 1), pattern(kind, world, 1u)));
    }
}

std::vector<uint32_t> partial(uint32_t world, uint32_t cap) {  // every rank something, nobody full: a rank that drops out or overruns shows
  std::vector<uint32_t> v(world);
  for (uint32_t r = 0; r < world; r++) v[r] = 1u + (37u * (r + 1u)) % (cap - 1u);
  return v;
}

void cases_truncated_and_failed() {
  const uint32_t cap = 300u;
  for (uint32_t world : {1u, 2u, 3u, 8u})
    for (int where = 0; where < 3; where++) {
      const uint32_t r = root_at(world, where), root = root_at(world, (where + 1) % 3);
      if ((where == 1 && world < 3u) || (where == 2 && world < 2u)) continue;
      const uint64_t seq = SEQ0 + (uint64_t)where;
      // the rank's list did not fit its message
      for (uint32_t count : {cap + 1u, 0xffffffffu}) {
        Post p = post_of(nm("truncated_w%u_%s_count%u", world, WHERE[where], count), seq, root, partial(world, cap));
        p.ranks[r] = good(seq, cap);
        p.ranks[r].pack.count = count;
        p.ranks[r].pack.status = (uint32_t)SCN_E_TRUNCATED;
        p.want_status = SCN_E_TRUNCATED;
        p.want_bad = (int)r;
        p.count_rank = (int)r;
        p.want_count = count;
        run_one(world, cap, p);
      }
      // the rank could not prepare its part: marked, empty
      Post p = post_of(nm("failed_w%u_%s", world, WHERE[where]), seq, root, partial(world, cap));
      p.ranks[r] = good(seq, 0u);
      p.ranks[r].pack.status = (uint32_t)SCN_E_NOMEM;
      p.want_status = SCN_E_COMM;
      p.want_bad = (int)r;
      run_one(world, cap, p);
      // intact, records behind it, but a status that is not OK: whatever scn_stream_outcome says is the definition (they are in the list)
      p = post_of(nm("marked_with_records_w%u_%s", world, WHERE[where]), seq, root, partial(world, cap));
      p.ranks[r].pack.status = (uint32_t)SCN_E_STATE;
      p.want_status = SCN_E_COMM;
      p.want_bad = (int)r;
      run_one(world, cap, p);
      // SCN_E_TRUNCATED with nothing cut off in the message (the plan's device list was shorter than its hits)
      p = post_of(nm("truncated_upstream_w%u_%s", world, WHERE[where]), seq, root, partial(world, cap));
      p.ranks[r].pack.status = (uint32_t)SCN_E_TRUNCATED;
      p.want_status = SCN_E_COMM;
      p.want_bad = (int)r;
      run_one(world, cap, p);
    }
}

enum Defect { MAGIC, SEQ_MINUS_1, SEQ_PLUS_1, SEQ_MINUS_TICKETS, SEQ_HIGH_WORD, SENT_CAP_PLUS_1, SENT_ABOVE_COUNT, SENT_MAX, N_DEFECTS };
const char *DEFECT[] = {"magic", "seqminus1", "seqplus1", "seqminustickets", "seqhighword", "sentcapplus1", "sentabovecount", "sentmax"};

// valid-looking records stay behind the header; what the pack kernel cannot safely be asked for is written over the header in the ring
void spoil(RankSpec &s, Defect d, uint64_t seq, uint32_t cap) {
  s.contributes = 0;
  switch (d) {
    case MAGIC: s.pack.magic = SCN_STREAM_MAGIC ^ 0x00010000u; break;
    case SEQ_MINUS_1: s.pack.seq = seq - 1u; break;
    case SEQ_PLUS_1: s.pack.seq = seq + 1u; break;
    case SEQ_MINUS_TICKETS: s.pack.seq = seq - SCN_GATHER_TICKETS; break;
    case SEQ_HIGH_WORD: s.pack.seq = seq ^ 0x100000000ull; break;
    case SENT_ABOVE_COUNT: s.pack.count = s.pack.sent - 1u; break;
    case SENT_CAP_PLUS_1:
      s.rewrite = true;
      s.ring_head = s.pack;
      s.ring_head.sent = s.ring_head.count = cap + 1u;
      break;
    case SENT_MAX:
      s.rewrite = true;
      s.ring_head = s.pack;
      s.ring_head.sent = 0xffffffffu;
      break;
    default: break;
  }
}

void cases_not_intact() {
  const uint32_t cap = 300u;
  for (uint32_t world : {1u, 2u, 3u, 8u})
    for (int d = 0; d < N_DEFECTS; d++)
      for (int where = 0; where < 3; where++) {
        if (where == 1 && world < 3u) continue;
        if (where == 2 && world < 2u) continue;
        const uint32_t r = root_at(world, where), root = root_at(world, (where + d) % 3);
        const uint64_t seq = SEQ0 + (uint64_t)((where + d) % 4);
        Post p = post_of(nm("bad_%s_w%u_%s", DEFECT[d], world, WHERE[where]), seq, root, partial(world, cap));
        spoil(p.ranks[r], (Defect)d, seq, cap);
        p.want_status = SCN_E_COMM;
        p.want_bad = (int)r;
        run_one(world, cap, p);
      }
  // several at once, next to each other and at both ends, beside full ranks
  for (int v = 0; v < 3; v++) {
    const uint64_t seq = SEQ0 + 2u;
    Post p = post_of(nm("bad_several_w8_%d", v), seq, root_at(8, v), std::vector<uint32_t>(8, v == 2 ? cap : cap - 1u));
    const uint32_t who[3][4] = {{0, 1, 4, 7}, {2, 3, 4, 6}, {0, 5, 6, 7}};
    for (int k = 0; k < 4; k++) spoil(p.ranks[who[v][k]], (Defect)((2 * k + v) % N_DEFECTS), seq, cap);
    p.want_status = SCN_E_COMM;
    p.want_bad = (int)who[v][0];
    run_one(8, cap, p);
  }
}

// SCN_GATHER_TICKETS posts in flight through one ring, one list buffer, one header buffer; then the same tickets again with a peer
// whose message does not arrive: its slot still holds the previous round's message, intact for seq - SCN_GATHER_TICKETS
void cases_ticket_ring() {
  for (uint32_t world : {2u, 3u, 8u})
    for (uint32_t cap : {300u, 683u}) {
      Session s(world, cap, SCN_GATHER_TICKETS);
      const uint32_t root = root_at(world, cap == 300u ? 1 : 2);
      const uint64_t seq0 = SEQ0 + 2u;  // the first post's ticket is 2: the ring wraps inside a round
      for (int round = 0; round < 2; round++) {
        std::vector<Post> posts;
        for (uint32_t k = 0; k < SCN_GATHER_TICKETS; k++) {
          const uint64_t seq = seq0 + (uint64_t)round * SCN_GATHER_TICKETS + k;
          std::vector<uint32_t> sent(world);
          for (uint32_t r = 0; r < world; r++) sent[r] = (r + k + round) % 4u == 0u ? cap : (97u * (r + 1u) + 13u * k + 5u * round) % cap;
          Post p = post_of(nm("ring_w%u_cap%u_round%d_post%u", world, cap, round, k), seq, root, sent);
          if (round == 1 && k % 2u == 1u) {
            const uint32_t lost = (root + 1u + (k / 2u) % (world - 1u)) % world;  // a peer, never the root
            if (lost == root) program_bug("the root's own message cannot be lost");
            p.ranks[lost].arrives = false;
            p.ranks[lost].contributes = 0;
            p.want_status = SCN_E_COMM;
            p.want_bad = (int)lost;
          }
          posts.push_back(p);
        }
        s.run(posts);
      }
    }
}
}  // namespace

int main(int argc, char **argv) {
  for (int k = 1; k + 1 < argc; k++)
    if (!strcmp(argv[k], "--only")) g_only = argv[k + 1];
  int n_dev = 0;
  HIP(hipGetDeviceCount(&n_dev));
  if (n_dev < 1) {
    printf("no HIP device\n");
    return 2;
  }
  HIP(hipSetDevice(0));
  cases_cap_edges();
  cases_sent_edges();
  cases_pack_grid();
  cases_patterns();
  cases_truncated_and_failed();
  cases_not_intact();
  cases_ticket_ring();
  printf("summary cases=%d failed=%d\n", g_cases, g_failed);
  return g_failed || !g_cases ? 1 : 0;
}
