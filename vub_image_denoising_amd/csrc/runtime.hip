// The library's own state and clocks: the thread's last error and the launch check every
// entry point ends with, the kernel-name probe of the conv / wgrad launchers, the version
// string, and the stream-ordered counter and wall-clock stamp a captured step replays.
#include <stdarg.h>
#include <stdio.h>

#include "rdn_pointwise.h"

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void rdn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int rdn_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    rdn_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return RDN_E_LAUNCH;
  }
  return RDN_OK;
}
extern "C" const char* rdn_last_error(void) { return g_err; }

thread_local char* rdn_probe_buf = nullptr;
thread_local int rdn_probe_len = 0;
thread_local int rdn_probe_rows = 0;
int rdn_probe_name(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(rdn_probe_buf, (size_t)rdn_probe_len, fmt, ap);
  va_end(ap);
  return RDN_OK;
}
extern "C" int rdn_conv_kernel_name(const rdn_conv_desc* d, char* buf, int32_t len) {
  if (!buf || len < 1) { rdn_set_error("rdn_conv_kernel_name: no buffer"); return RDN_E_ARG; }
  buf[0] = 0;
  rdn_probe_buf = buf;
  rdn_probe_len = len;
  const int rc = rdn_conv_fwd(d, nullptr);
  rdn_probe_buf = nullptr;
  return rc;
}
extern "C" int rdn_conv_gate_rows(const rdn_conv_desc* d) {
  if (!d || !d->gout) return 0;
  char buf[128];
  rdn_probe_buf = buf;
  rdn_probe_len = (int)sizeof(buf);
  rdn_probe_rows = 0;
  const int rc = rdn_conv_fwd(d, nullptr);
  rdn_probe_buf = nullptr;
  return rc == RDN_OK ? rdn_probe_rows : 0;
}
extern "C" int rdn_wgrad_kernel_name(const rdn_wgrad_desc* d, char* buf, int32_t len) {
  if (!buf || len < 1) { rdn_set_error("rdn_wgrad_kernel_name: no buffer"); return RDN_E_ARG; }
  buf[0] = 0;
  rdn_probe_buf = buf;
  rdn_probe_len = len;
  const int rc = rdn_conv_wgrad(d, nullptr);
  rdn_probe_buf = nullptr;
  return rc;
}
extern "C" const char* rdn_version(void) { return "rdunet_hip 0.1.0 gfx950"; }

namespace {

__global__ void counter_inc_kernel(int64_t* c) { *c += 1; }

// the device's constant-rate wall clock when this kernel starts, by one lane (vector
// store): stream-ordered timestamps that a captured hipGraph replays (bench.py's
// exposed all-reduce time of the replayed data-parallel step)
__global__ void stamp_kernel(uint64_t* buf, int slot) {
  if (threadIdx.x == 0) buf[slot] = wall_clock64();
}

}  // namespace

extern "C" int rdn_counter_inc(int64_t* counter, void* stream) {
  if (!counter) { rdn_set_error("rdn_counter_inc: null"); return RDN_E_ARG; }
  counter_inc_kernel<<<1, 1, 0, RDN_STREAM>>>(counter);
  return rdn_check_launch("rdn_counter_inc");
}

extern "C" int rdn_stamp(uint64_t* buf, int32_t slot, void* stream) {
  if (!buf || slot < 0) { rdn_set_error("rdn_stamp: bad arguments"); return RDN_E_ARG; }
  stamp_kernel<<<1, 64, 0, RDN_STREAM>>>(buf, slot);
  return rdn_check_launch("rdn_stamp");
}

extern "C" int64_t rdn_wall_clock_khz(void) {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
      khz <= 0) {
    rdn_set_error("rdn_wall_clock_khz: no device clock rate");
    return RDN_E_LAUNCH;
  }
  return khz;
}
