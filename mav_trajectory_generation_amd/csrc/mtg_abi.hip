// mtg_abi.hip -- the C ABI of include/mtg_hip.h, part 1: status strings, the context and its options, device-memory helpers,
// mtg_context_sync, the layouts and the pivot-reciprocal self-test.  The other parts: mtg_plan.hip, mtg_dispatch.hip,
// mtg_shadow.hip, mtg_multi.hip (shared declarations: mtg_abi_internal.h); the kernels live in mtg_kernels.h and its kin.
#include "mtg_abi_internal.h"

namespace {
// accuracy probe of the pivot reciprocal (mtg_selftest_rcp)
__global__ void mtg_rcp_selftest_kernel(int n, double* out, int iters) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double err = 0.0;
  if (i < n) {
    // deterministic pseudo-random positive doubles over ~24 binades
    unsigned long long z = 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
    z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
    const double m = 1.0 + (double)(z >> 11) * (1.0 / 9007199254740992.0);
    const int e = (int)((z & 0x3FF) % 49) - 24;
    const double x = ldexp(m, e);
    double r;
    if (iters == 2) {
      r = mtg_rcp(x);
    } else {
      r = __builtin_amdgcn_rcp(x);
      for (int it = 0; it < iters; ++it) r = mtg_fma(mtg_fma(-x, r, 1.0), r, r);
    }
    const double ref = 1.0 / x;
    err = fabs(r - ref) / ref;
  }
  // block max -> atomic max on the bit pattern (values are non-negative)
  __shared__ double sm[256];
  sm[threadIdx.x] = err;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax((unsigned long long*)out, (unsigned long long)__double_as_longlong(sm[0]));
}
}  // namespace

int mtg_status_code(mtg_context* ctx, int st) {
  if (st & MTG_FLAG_BAD_TIME) return set_err(ctx, MTG_ERR_BAD_SEGMENT_TIME, mtg_status_string(MTG_ERR_BAD_SEGMENT_TIME));
  if (st & MTG_FLAG_SINGULAR) return set_err(ctx, MTG_ERR_SINGULAR, mtg_status_string(MTG_ERR_SINGULAR));
  return MTG_OK;
}

extern "C" {
const char* mtg_status_string(int status) {
  switch (status) {
    case MTG_OK: return "ok";
    case MTG_ERR_INVALID_ARGUMENT: return "invalid argument";
    case MTG_ERR_BAD_SEGMENT_TIME: return "segment times need to be greater than zero";
    case MTG_ERR_SINGULAR: return "non-positive pivot: free-constraint system is rank deficient";
    case MTG_ERR_DEVICE: return "HIP runtime error";
    case MTG_ERR_NO_DEVICE: return "no usable HIP device";
    case MTG_ERR_UNSUPPORTED: return "unsupported configuration";
  }
  return "unknown status";
}

const char* mtg_last_error_string(const mtg_context* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int mtg_context_create(int device, void* stream, mtg_context** out) {
  if (!out) return MTG_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return MTG_ERR_NO_DEVICE;
  mtg_context* ctx = new (std::nothrow) mtg_context();
  if (!ctx) return MTG_ERR_DEVICE;
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess) { delete ctx; return MTG_ERR_NO_DEVICE; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
  if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return MTG_ERR_DEVICE; }
    ctx->own_stream = true;
  }
  if (hipMalloc((void**)&ctx->d_status, sizeof(int)) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_status, sizeof(int), hipHostMallocDefault) != hipSuccess ||
      hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream) != hipSuccess) {
    mtg_context_destroy(ctx);
    return MTG_ERR_DEVICE;
  }
  *ctx->h_status = 0;
  *out = ctx;
  return MTG_OK;
}

// include/mtg_hip_lab.h: measurement knobs by name (no environment reads inside the library)
int mtg_context_set_option(mtg_context* ctx, const char* name, int value) {
  if (!ctx || !name) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const std::string n(name);
  if (n == "force_dg") ctx->knobs.force_dg = value;
  else if (n == "prefer_rolled") ctx->knobs.prefer_rolled = value != 0;
  else if (n == "no_dimlane") ctx->knobs.no_dimlane = value != 0;
  else if (n == "no_slab") ctx->knobs.no_slab = value != 0;
  else if (n == "no_queue") ctx->knobs.no_queue = value != 0;
  else if (n == "no_slab_extra") ctx->knobs.no_slab_extra = value != 0;
  else if (n == "no_dl_extra") ctx->knobs.no_dl_extra = value != 0;
  else if (n == "no_balance") ctx->knobs.no_balance = value != 0;
  else if (n == "dl_rt") ctx->knobs.dl_rt = value;
  else if (n == "dl_grid_per_cu") ctx->knobs.dl_grid_per_cu = std::max(1, value);
  else if (n == "dl_any_sched_rr") ctx->knob_dl_any_rr = value != 0;
  else if (n == "slab_policy") ctx->knobs.slab_policy = value < 0 ? -1 : (value ? 1 : 0);
  else if (n == "rolled_wg_per_cu") ctx->knobs.rolled_wg_per_cu = std::max(1, value);
  else if (n == "dl_max_units") ctx->knobs.dl_max_units_per_cu = value;
  else if (n == "sample_generic") ctx->knob_sample_generic = value != 0;
  else if (n == "sample_max_blocks") ctx->knob_sample_max_blocks = std::max(0, value);
  else if (n == "coop") ctx->knobs.coop = value;
  else if (n == "extrema_split") ctx->knob_extrema_split = value;
  else if (n == "field_lanes") ctx->knob_field_lanes = (value == 1 || value == 4 || value == 16 || value == 64) ? value : 0;
  else return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "unknown option: " + n);
  return MTG_OK;
}

// (mtg_sample.hip, mtg_extrema.hip, mtg_field.hip)
bool mtg_context_sample_generic(const mtg_context* ctx) { return ctx && ctx->knob_sample_generic; }
int mtg_context_sample_max_blocks(const mtg_context* ctx) { return ctx ? ctx->knob_sample_max_blocks : 0; }
int mtg_context_extrema_split(const mtg_context* ctx) { return ctx ? ctx->knob_extrema_split : -1; }
int mtg_context_field_lanes(const mtg_context* ctx) { return ctx ? ctx->knob_field_lanes : 0; }

int mtg_context_destroy(mtg_context* ctx) {
  if (!ctx) return MTG_OK;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  if (ctx->d_status) hipFree(ctx->d_status);
  if (ctx->h_status) hipHostFree(ctx->h_status);
  if (ctx->h_bounce) hipHostFree(ctx->h_bounce);
  if (ctx->own_stream) hipStreamDestroy(ctx->stream);
  for (hipStream_t q : ctx->side_streams) { hipStreamSynchronize(q); hipStreamDestroy(q); }
  for (hipEvent_t e : ctx->join_events) hipEventDestroy(e);
  if (ctx->fork_event) hipEventDestroy(ctx->fork_event);
  for (auto& sc : ctx->dl_any_schedules) { if (sc.d_units) hipFree(sc.d_units); if (sc.d_wg_begin) hipFree(sc.d_wg_begin); }
  if (ctx->dl_any_ws) hipFree(ctx->dl_any_ws);
  for (auto& pb : ctx->dl_any_item_pool) hipFree(pb.first);
  delete ctx;
  return MTG_OK;
}

// used by the other translation units of the library (mtg_sample.hip): the context's stream and device
int mtg_context_stream_device(mtg_context* ctx, void** stream, int* device) {
  if (!ctx || !stream || !device) return MTG_ERR_INVALID_ARGUMENT;
  *stream = (void*)ctx->stream;
  *device = ctx->device;
  return MTG_OK;
}

// ... and the context's error text (mtg_feasibility.hip: argument errors say which argument)
int mtg_context_set_last_error(mtg_context* ctx, int code, const char* message) { return set_err(ctx, code, message ? message : ""); }

// ---- device memory helpers: host code above the C ABI never sees HIP headers ---------------------------------
int mtg_device_malloc(mtg_context* ctx, size_t bytes, void** device_ptr) {
  if (!ctx || !device_ptr) return MTG_ERR_INVALID_ARGUMENT;
  *device_ptr = nullptr;
  if (bytes == 0) return MTG_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipMalloc(device_ptr, bytes));
  return MTG_OK;
}

int mtg_device_free(mtg_context* ctx, void* device_ptr) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!device_ptr) return MTG_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // nothing queued on the context may still use it
  MTG_HIP_TRY(ctx, hipFree(device_ptr));
  return MTG_OK;
}

int mtg_copy_to_device(mtg_context* ctx, void* dst_device, const void* src_host, size_t bytes) {
  if (!ctx || (bytes && (!dst_device || !src_host))) return MTG_ERR_INVALID_ARGUMENT;
  if (bytes == 0) return MTG_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the host buffer may be reused on return
  return MTG_OK;
}

int mtg_copy_to_host(mtg_context* ctx, void* dst_host, const void* src_device, size_t bytes) {
  if (!ctx || (bytes && (!dst_host || !src_device))) return MTG_ERR_INVALID_ARGUMENT;
  if (bytes == 0) return MTG_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, ctx->stream));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MTG_OK;
}

// The device status word is fetched on EVERY sync (one 4-byte copy): kernels replayed from a captured hipGraph never
// pass through the library, so no host-side bookkeeping can know whether flags were raised since the last sync.
int mtg_context_sync(mtg_context* ctx) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  MTG_HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0, sizeof(int), ctx->stream));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return mtg_status_code(ctx, *ctx->h_status);
}

void mtg_layout_aos(const mtg_plan* p, int64_t batch, mtg_layout* L) {
  (void)batch;
  L->times_stride_b = p->K; L->times_stride_k = 1;
  mtg_fixed_contiguous(L, p->D, p->n_fixed);
  mtg_free_contiguous(L, p->D, p->n_free);
}

// SoA with row stride bs: times[K][bs], d_fixed[D][n_fixed][bs], d_free[D][n_free][bs]
static void layout_soa_rows(const mtg_plan* p, int64_t bs, mtg_layout* L) {
  L->times_stride_b = 1; L->times_stride_k = bs;
  L->fixed_stride_b = 1; L->fixed_stride_d = (int64_t)p->n_fixed * bs; L->fixed_stride_c = bs;
  L->free_stride_b = 1; L->free_stride_d = (int64_t)p->n_free * bs; L->free_stride_c = bs;
}
void mtg_layout_soa_padded(const mtg_plan* p, int64_t batch, mtg_layout* L) { layout_soa_rows(p, mtg_padded16(batch), L); }
void mtg_layout_soa(const mtg_plan* p, int64_t batch, mtg_layout* L) { layout_soa_rows(p, batch, L); }

int mtg_selftest_rcp(mtg_context* ctx, int n, double* max_rel_err) {
  if (!ctx || !max_rel_err || n == 0) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  double* d = nullptr;
  MTG_HIP_TRY(ctx, hipMalloc((void**)&d, sizeof(double)));
  MTG_HIP_TRY(ctx, hipMemsetAsync(d, 0, sizeof(double), ctx->stream));
  hipLaunchKernelGGL(mtg_rcp_selftest_kernel, dim3((std::abs(n) + 255) / 256), dim3(256), 0, ctx->stream, std::abs(n), d, n < 0 ? ((-n) & 3) : 2);
  MTG_HIP_TRY(ctx, hipMemcpyAsync(max_rel_err, d, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  MTG_HIP_TRY(ctx, hipFree(d));
  return MTG_OK;
}
}  // extern "C"
