// scn_welch_plan.hip -- the Welch PSD plan (BASELINE C5) of the C-ABI: scn_welch* on top of the kernels of scn_welch.hip.
#include <cstring>
#include <new>
#include <vector>

#include "scn_plan.h"

namespace {
// What the two kernels of a submit pass between them
struct WelchWork {
  ScnDeviceMem<char> d_work;      // [max_psd*K][n] complex
  ScnDeviceMem<float> d_partial;  // [parts][max_psd][n] partial power sums (row kernel -> combine kernel), parts > 1
  ScnDeviceMem<int> d_dc;         // [max_psd*K + 1][2] block sums (correct_dc on an integer wire format)
  hipError_t alloc(const scn_welch *w);
};

struct WelchSlot {
  ~WelchSlot() {
    if (graph) (void)hipGraphExecDestroy(graph);
  }
  ScnStream stream;                // the pinned path's own stream: this slot's H2D overlaps the other slot's kernels (first: destroyed last)
  ScnPinnedMem<char> h_in;         // pinned samples
  ScnPinnedMem<float> h_psd;       // pinned results (graph path)
  ScnDeviceMem<char> d_in;
  ScnDeviceMem<float> d_psd;
  float *cur_psd = nullptr;        // device location of the pending results (d_psd or the caller's)
  bool via_graph = false;
  hipGraphExec_t graph = nullptr;  // captured H2D -> kernel A -> kernel B -> D2H for graph_npsd PSDs
  WelchWork work;                  // ... which needs a work set of its own
  uint32_t graph_npsd = 0;
  ScnEvent done;
  SlotLife life;                   // (of which a Welch slot has `pending` alone)
  uint32_t n_psd = 0;
};
}  // namespace

struct scn_welch : WelchShape {  // (resolve_welch, scn_host.hip: the descriptor and what follows from it alone)
  ScnStream stream;  // (first: destroyed after the slots and the memory used on it)
  int num_cus = 0;
  ScnDeviceMem<float> d_window;
  ScnDeviceMem<scn_v2f> d_twiddle;
  WelchWork work;  // the device path's: shared by the slots through stream order (the pinned path's slots own theirs)
  uint32_t parts = 1;
  ScnDeviceMem<double> d_tw256;  // W_256^m in double (the row transform)
  WelchSlot slot[SCN_NUM_SLOTS];
};

namespace {
hipError_t WelchWork::alloc(const scn_welch *w) {
  const size_t segments = (size_t)w->d.max_psd * w->d.segments_per_psd;
  hipError_t e = d_work.alloc(sizeof(float) * 2 * w->d.n * segments);
  if (e == hipSuccess && w->parts > 1) e = d_partial.alloc((size_t)w->d.n * w->d.max_psd * w->parts);
  if (e == hipSuccess && w->dc) e = d_dc.alloc(2u * (segments + 1u));
  return e;
}

size_t welch_samples(const scn_welch *w, uint32_t n_psd) {
  return ((size_t)n_psd * w->d.segments_per_psd + 1u) * w->hop;
}

int welch_enqueue(scn_welch *w, const void *d_in, uint32_t n_psd, float *d_psd, hipStream_t stream, const WelchWork &work) {
  ScnWelchArgs a;
  a.scale = w->scale;
  a.dc_sums = work.d_dc.get();
  a.tw256 = reinterpret_cast<const double2_scn *>(w->d_tw256.get());
  a.partial = work.d_partial.get();
  a.parts = w->parts;
  a.in = d_in;
  a.window = w->d_window.get();
  a.twiddle = w->d_twiddle.get();
  a.work = work.d_work.get();
  a.psd_db = d_psd;
  a.n_segments = n_psd * w->d.segments_per_psd;
  a.hop = w->hop;
  a.k = w->d.segments_per_psd;
  a.n_psd = n_psd;
  a.inv_k = 1.0f / (float)w->d.segments_per_psd;
  SCN_HIP(scn_launch_welch((int)w->d.sample_kind, w->dc, a, w->num_cus, stream));
  return SCN_OK;
}

int welch_check(scn_welch *w, int slot) {
  if (!w) return scn_fail(SCN_E_INVALID, "null welch plan");
  if (slot < 0 || slot >= SCN_NUM_SLOTS) return scn_fail(SCN_E_INVALID, "slot %d out of range", slot);
  return SCN_OK;
}
}  // namespace

extern "C" {

int scn_welch_create(const scn_welch_desc *desc, scn_welch **out) {
  if (!desc || !out) return scn_fail(SCN_E_INVALID, "null argument");
  *out = nullptr;
  WelchShape shape;
  if (int st = resolve_welch(desc, &shape)) return st;
  const scn_welch_desc &d = shape.d;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return scn_fail(SCN_E_NO_DEVICE, "no HIP device visible");
  if (d.device_id < 0 || d.device_id >= ndev) return scn_fail(SCN_E_INVALID, "device_id %d out of range", d.device_id);
  SCN_HIP(hipSetDevice(d.device_id));
  scn_welch *w = new (std::nothrow) scn_welch();
  if (!w) return scn_fail(SCN_E_NOMEM, "out of host memory");
  static_cast<WelchShape &>(*w) = shape;
  std::vector<float> win;
  build_window(d.window_type, d.n, win);
  hipDeviceProp_t prop;
  hipError_t e = hipSuccess;
  do {
    if ((e = hipGetDeviceProperties(&prop, d.device_id)) != hipSuccess) break;
    w->num_cus = prop.multiProcessorCount;
    if ((e = w->stream.create()) != hipSuccess) break;
    if ((e = upload(w->d_window, win)) != hipSuccess) break;
    if ((e = upload(w->d_twiddle, twiddles<float>(d.n))) != hipSuccess) break;
    if ((e = upload(w->d_tw256, twiddles<double>(256))) != hipSuccess) break;
    w->parts = welch_parts(d.max_psd, d.segments_per_psd, w->num_cus);
    e = w->work.alloc(w);
  } while (0);
  if (e != hipSuccess) {
    int st = scn_fail(e == hipErrorOutOfMemory ? SCN_E_NOMEM : SCN_E_HIP, "scn_welch_create: %s", hipGetErrorString(e));
    scn_welch_destroy(w);
    return st;
  }
  *out = w;
  return SCN_OK;
}

int scn_welch_destroy(scn_welch *w) {
  if (!w) return SCN_OK;
  (void)hipSetDevice(w->d.device_id);  // the members are released with the plan's device current, nothing of the plan's still running
  w->stream.sync();
  for (int i = 0; i < SCN_NUM_SLOTS; i++) w->slot[i].stream.sync();
  delete w;
  return SCN_OK;
}

int scn_welch_samples(const scn_welch *w, uint32_t n_psd, size_t *n_samples) {
  if (!w || !n_samples) return scn_fail(SCN_E_INVALID, "null argument");
  *n_samples = welch_samples(w, n_psd);
  return SCN_OK;
}

int scn_welch_partition(const scn_welch *w, uint32_t n_psd, uint32_t *parts, uint32_t *column_groups, uint32_t *segments_per_group) {
  if (!w) return scn_fail(SCN_E_INVALID, "null welch plan");
  if (n_psd < 1 || n_psd > w->d.max_psd) return scn_fail(SCN_E_INVALID, "n_psd %u out of range (1..%u)", n_psd, w->d.max_psd);
  uint32_t groups = 0, per = 0;
  scn_welch_column_groups(n_psd * w->d.segments_per_psd, w->num_cus, &groups, &per);
  if (parts) *parts = w->parts;
  if (column_groups) *column_groups = groups;
  if (segments_per_group) *segments_per_group = per;
  return SCN_OK;
}

int scn_welch_host_buffer(scn_welch *w, int slot, void **ptr, size_t *bytes) {
  if (int st = welch_check(w, slot)) return st;
  if (!ptr) return scn_fail(SCN_E_INVALID, "null argument");
  WelchSlot &s = w->slot[slot];
  SCN_HIP(hipSetDevice(w->d.device_id));
  const size_t total = welch_samples(w, w->d.max_psd) * w->bytes_per_sample;
  SCN_HIP(s.h_in.alloc(total));
  *ptr = s.h_in.get();
  if (bytes) *bytes = total;
  return SCN_OK;
}

int scn_welch_submit(scn_welch *w, int slot, uint32_t n_psd) {
  if (int st = welch_check(w, slot)) return st;
  WelchSlot &s = w->slot[slot];
  if (n_psd < 1 || n_psd > w->d.max_psd) return scn_fail(SCN_E_INVALID, "n_psd %u out of range (1..%u)", n_psd, w->d.max_psd);
  if (int st = require_free(s.life, slot)) return st;
  if (!s.h_in) return scn_fail(SCN_E_STATE, "slot %d: scn_welch_host_buffer was never called", slot);
  SCN_HIP(hipSetDevice(w->d.device_id));
  const size_t in_bytes = welch_samples(w, w->d.max_psd) * w->bytes_per_sample, psd_floats = (size_t)w->d.n * w->d.max_psd;
  SCN_HIP(s.d_in.alloc(in_bytes));
  SCN_HIP(s.d_psd.alloc(psd_floats));
  SCN_HIP(s.h_psd.alloc(psd_floats));
  SCN_HIP(s.done.create());
  SCN_HIP(s.stream.create());
  SCN_HIP(s.work.alloc(w));
  hipStream_t stream = s.stream.get();
  if (!s.graph || s.graph_npsd != n_psd) {
    // capture the slot's inner loop once per batch size: H2D -> columns -> rows -> D2H
    if (s.graph) {
      (void)hipGraphExecDestroy(s.graph);
      s.graph = nullptr;
    }
    hipGraph_t graph = nullptr;
    SCN_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    hipError_t e = hipMemcpyAsync(s.d_in.get(), s.h_in.get(), welch_samples(w, n_psd) * w->bytes_per_sample, hipMemcpyHostToDevice, stream);
    int inner = SCN_OK;
    if (e == hipSuccess) inner = welch_enqueue(w, s.d_in.get(), n_psd, s.d_psd.get(), stream, s.work);
    if (e == hipSuccess && inner == SCN_OK)
      e = hipMemcpyAsync(s.h_psd.get(), s.d_psd.get(), sizeof(float) * (size_t)w->d.n * n_psd, hipMemcpyDeviceToHost, stream);
    hipError_t e2 = hipStreamEndCapture(stream, &graph);
    if (e != hipSuccess || e2 != hipSuccess || inner != SCN_OK) {
      if (graph) (void)hipGraphDestroy(graph);
      if (inner != SCN_OK) return inner;
      return scn_fail(SCN_E_HIP, "Welch graph capture failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    e = hipGraphInstantiate(&s.graph, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return scn_fail(SCN_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    s.graph_npsd = n_psd;
  }
  SCN_HIP(hipGraphLaunch(s.graph, stream));
  SCN_HIP(hipEventRecord(s.done.get(), stream));
  on_submitted(s.life);
  s.via_graph = true;
  s.n_psd = n_psd;
  s.cur_psd = s.d_psd.get();
  return SCN_OK;
}

int scn_welch_submit_device(scn_welch *w, int slot, const void *d_samples, uint32_t n_psd, float *d_psd_db) {
  int st = welch_check(w, slot);
  if (st) return st;
  WelchSlot &s = w->slot[slot];
  if (n_psd < 1 || n_psd > w->d.max_psd) return scn_fail(SCN_E_INVALID, "n_psd %u out of range (1..%u)", n_psd, w->d.max_psd);
  if (!d_samples) return scn_fail(SCN_E_INVALID, "null argument");
  if (int st = require_free(s.life, slot)) return st;
  SCN_HIP(hipSetDevice(w->d.device_id));
  if (!d_psd_db) {
    SCN_HIP(s.d_psd.alloc((size_t)w->d.n * w->d.max_psd));
    d_psd_db = s.d_psd.get();
  }
  SCN_HIP(s.done.create());
  st = welch_enqueue(w, d_samples, n_psd, d_psd_db, w->stream.get(), w->work);
  if (st) return st;
  SCN_HIP(hipEventRecord(s.done.get(), w->stream.get()));
  on_submitted(s.life);
  s.via_graph = false;
  s.n_psd = n_psd;
  s.cur_psd = d_psd_db;
  return SCN_OK;
}

int scn_welch_collect(scn_welch *w, int slot, float *psd_db) {
  if (int st = welch_check(w, slot)) return st;
  WelchSlot &s = w->slot[slot];
  if (int st = require_pending(s.life, slot)) return st;
  SCN_HIP(hipSetDevice(w->d.device_id));
  SCN_HIP(hipEventSynchronize(s.done.get()));
  on_take(s.life);
  if (psd_db) {
    const size_t bytes = sizeof(float) * (size_t)w->d.n * s.n_psd;
    if (s.via_graph) {
      memcpy(psd_db, s.h_psd.get(), bytes);  // the graph already brought the PSDs to pinned memory
    } else {
      SCN_HIP(hipMemcpyAsync(psd_db, s.cur_psd, bytes, hipMemcpyDeviceToHost, w->stream.get()));
      SCN_HIP(hipStreamSynchronize(w->stream.get()));
    }
  }
  return SCN_OK;
}

}  // extern "C"
