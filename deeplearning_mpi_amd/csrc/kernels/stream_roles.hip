// Per-device, per-stream-ROLE device workspaces that launchers may not allocate themselves (a launch
// can be inside a hipGraph capture): the last-arriver tickets of the fused BN finalize (bn.hip
// colsum_fin_kernel) and the split-K slab and tickets of the conv kernel (conv_igemm.hip).
// Launches on one stream are serialised, so they can share a workspace; the engine's auxiliary
// streams (models/engine.py: the weight-gradient side stream and the residual-branch stream) run
// concurrently with the main stream's, so each role gets its own.  (Per role rather than per
// stream: a graph capture runs the main role on a fresh capture stream, where no allocation may
// happen.)
#include "common.h"

constexpr int kRoles = 4;   // 0 = main (any unregistered stream), 1..3 = registered aux streams
constexpr int kMaxDev = 64;
static hipStream_t g_aux_stream[kMaxDev][kRoles] = {};

static bool cur_device(int* dev) { return hipGetDevice(dev) == hipSuccess && *dev >= 0 && *dev < kMaxDev; }

static int role_of(hipStream_t s, int dev) {
  for (int r = 1; r < kRoles; ++r)
    if (s != nullptr && s == g_aux_stream[dev][r]) return r;
  return 0;
}

static bool capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone;
}

// Self-resetting per-channel-group tickets of colsum_fin_kernel, one array of kFinTickets per role,
// zeroed once (the first use happens before any hipGraph capture: the warm-up steps run eagerly).
constexpr int kFinTickets = 4096;
static int* g_tickets[kMaxDev] = {};

static int* tickets_for_device(int dev) {
  if (!g_tickets[dev]) {
    int* p = nullptr;
    if (hipMalloc(&p, kRoles * kFinTickets * sizeof(int)) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, kRoles * kFinTickets * sizeof(int)) != hipSuccess) return nullptr;
    g_tickets[dev] = p;
  }
  return g_tickets[dev];
}

namespace dlmpi {
int* fin_tickets(hipStream_t s) {
  int dev = 0;
  if (!cur_device(&dev)) return nullptr;
  int* t = tickets_for_device(dev);
  return t ? t + role_of(s, dev) * kFinTickets : nullptr;
}
}  // namespace dlmpi

extern "C" hipError_t dlmpi_set_aux_stream(hipStream_t s, int role) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= kMaxDev || role < 1 || role >= kRoles || !tickets_for_device(dev))
    return hipErrorInvalidValue;   // (allocates outside any capture)
  g_aux_stream[dev][role] = s;
  return hipSuccess;
}

// Split-K workspaces of the conv kernel.  The slab grows on demand outside graph captures (the eager
// warm-up steps size it); inside a capture a too-small slab makes the launcher fall back to no split.
static float* g_sk_slab[kMaxDev][kRoles] = {};
static size_t g_sk_slab_floats[kMaxDev][kRoles] = {};
static int* g_sk_tk[kMaxDev][kRoles] = {};
constexpr int kSplitTickets = 4096;

extern "C" float* dlmpi_splitk_slab(hipStream_t s, size_t floats) {
  int dev = 0;
  if (!cur_device(&dev)) return nullptr;
  const int r = role_of(s, dev);
  if (g_sk_slab_floats[dev][r] >= floats) return g_sk_slab[dev][r];
  if (capturing(s)) return nullptr;
  // the old slab is never freed: a captured hipGraph may still reference it (a few MB, kept)
  const size_t n = floats + floats / 2;   // head room
  float* p = nullptr;
  if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) return nullptr;
  g_sk_slab[dev][r] = p;
  g_sk_slab_floats[dev][r] = n;
  return p;
}

extern "C" int* dlmpi_splitk_tickets(hipStream_t s, int n) {
  int dev = 0;
  if (n > kSplitTickets || !cur_device(&dev)) return nullptr;
  const int r = role_of(s, dev);
  if (!g_sk_tk[dev][r]) {
    if (capturing(s)) return nullptr;
    int* p = nullptr;
    if (hipMalloc(&p, kSplitTickets * sizeof(int)) != hipSuccess) return nullptr;
    if (hipMemsetAsync(p, 0, kSplitTickets * sizeof(int), s) != hipSuccess) return nullptr;   // ordered before the kernel
    g_sk_tk[dev][r] = p;
  }
  return g_sk_tk[dev][r];
}
