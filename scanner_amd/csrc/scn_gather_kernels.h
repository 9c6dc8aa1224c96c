// scn_gather_kernels.h -- the two kernels of the steady-state gather (scn_gather_post / scn_gather_wait, scn_gather.hip) with
// the host arithmetic that launches and addresses them: grids, a message's place in the ring, a ticket's place in the outgoing
// buffer and in the pinned list / headers.  scn_gather_post uses these functions and nothing else for those purposes, so that
// tests/cpp/test_gather_kernels_gpu.cpp -- a stand-alone program that fills the ring with what `world` ranks would have sent --
// runs the production grids and addresses at world sizes above one, not a copy of them.  No RCCL here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "scn_gather_protocol.h"

// message = [header][cap records]; the first `h.sent` records of `src` follow the header
static __global__ __launch_bounds__(256) void scn_gather_pack_kernel(const scn_hit *src, ScnStreamHeader h, scn_hit *msg) {
  typedef unsigned long long u64;
  const u64 *s = reinterpret_cast<const u64 *>(src);
  u64 *d = reinterpret_cast<u64 *>(msg + 1);
  const size_t words = (size_t)h.sent * 3u;  // 24-byte records as three 8-byte words: coalesced
  for (size_t e = (size_t)blockIdx.x * 256u + threadIdx.x; e < words; e += (size_t)gridDim.x * 256u) d[e] = s[e];
  if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<ScnStreamHeader *>(msg) = h;
}

// root: the world's messages [world][cap + 1] -> the rank-major list and the headers, both in pinned host memory.
// grid = world x chunks; workgroup (r, c) finds rank r's place from the headers before it (world is a node's GPU count).
static __global__ __launch_bounds__(256) void scn_gather_compact_kernel(const scn_hit *ring, uint32_t world, uint32_t cap, uint64_t seq, scn_hit *list,
                                                                         ScnStreamHeader *heads) {
  typedef unsigned long long u64;
  const uint32_t r = blockIdx.x % world, chunk = blockIdx.x / world, chunks = gridDim.x / world;
  auto sent_of = [&](uint32_t q) -> uint32_t {
    const ScnStreamHeader h = *reinterpret_cast<const ScnStreamHeader *>(ring + (size_t)q * (cap + 1u));
    // as scn_stream_outcome reads it: held to that function, byte for byte, by tests/cpp/test_gather_kernels_gpu.cpp
    return (h.magic == SCN_STREAM_MAGIC && h.seq == seq && h.sent <= cap && h.sent <= h.count) ? h.sent : 0u;
  };
  size_t off = 0;
  for (uint32_t q = 0; q < r; q++) off += sent_of(q);
  const size_t words = (size_t)sent_of(r) * 3u;
  const u64 *s = reinterpret_cast<const u64 *>(ring + (size_t)r * (cap + 1u) + 1u);
  u64 *d = reinterpret_cast<u64 *>(list + off);
  for (size_t e = (size_t)chunk * 256u + threadIdx.x; e < words; e += (size_t)chunks * 256u) d[e] = s[e];
  if (chunk == 0 && threadIdx.x == 0) heads[r] = *reinterpret_cast<const ScnStreamHeader *>(ring + (size_t)r * (cap + 1u));
}

// ---- grids ------------------------------------------------------------------------------------------------------------------
// pack: a workgroup per 256 words of the `sent` records, 64 at the most (the kernel strides over the rest), one for an empty list
inline uint32_t scn_gather_pack_blocks(uint32_t sent) {
  const uint32_t want = (sent * 3u + 255u) / 256u;
  return sent ? (want < 64u ? want : 64u) : 1u;
}

// compaction: per rank a chunk per 2048 words of a full message, between 1 and 16
inline uint32_t scn_gather_compact_chunks(uint32_t cap) {
  const uint32_t want = (cap * 3u + 2047u) / 2048u;
  return want < 1u ? 1u : want > 16u ? 16u : want;
}
inline uint32_t scn_gather_compact_blocks(uint32_t world, uint32_t cap) { return world * scn_gather_compact_chunks(cap); }

// ---- places (all in records of their buffer) ----------------------------------------------------------------------------------
inline size_t scn_gather_msg_records(uint32_t cap) { return (size_t)cap + 1u; }  // the header takes one record's place
// rank r's message of ticket tk in the root's ring [SCN_GATHER_TICKETS][world][cap + 1]
inline size_t scn_gather_ring_at(uint32_t tk, uint32_t world, uint32_t r, uint32_t cap) { return ((size_t)tk * world + r) * scn_gather_msg_records(cap); }
// ticket tk's message in a rank's outgoing buffer [SCN_GATHER_TICKETS][cap + 1]
inline size_t scn_gather_out_at(uint32_t tk, uint32_t cap) { return (size_t)tk * scn_gather_msg_records(cap); }
// ticket tk's list in the pinned lists [SCN_GATHER_TICKETS][world * cap] and its headers in the pinned [SCN_GATHER_TICKETS][world]
inline size_t scn_gather_list_at(uint32_t tk, uint32_t world, uint32_t cap) { return (size_t)tk * cap * world; }
inline size_t scn_gather_heads_at(uint32_t tk, uint32_t world) { return (size_t)tk * world; }

// ---- launchers ----------------------------------------------------------------------------------------------------------------
// `msg`: where the message goes (cap + 1 records of room, of which 1 + h.sent are written); `src` may be null when h.sent == 0
inline hipError_t scn_launch_gather_pack(const scn_hit *src, const ScnStreamHeader &h, scn_hit *msg, hipStream_t stream) {
  hipLaunchKernelGGL(scn_gather_pack_kernel, dim3(scn_gather_pack_blocks(h.sent)), dim3(256), 0, stream, src, h, msg);
  return hipGetLastError();
}

// `ring`: the first message of the post's ticket (scn_gather_ring_at(tk, world, 0, cap)); `list` / `heads`: the ticket's own
inline hipError_t scn_launch_gather_compact(const scn_hit *ring, uint32_t world, uint32_t cap, uint64_t seq, scn_hit *list, ScnStreamHeader *heads,
                                            hipStream_t stream) {
  hipLaunchKernelGGL(scn_gather_compact_kernel, dim3(scn_gather_compact_blocks(world, cap)), dim3(256), 0, stream, ring, world, cap, seq, list, heads);
  return hipGetLastError();
}
