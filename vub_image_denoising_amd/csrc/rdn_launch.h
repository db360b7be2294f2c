// Host-side launch helpers shared by the kernel files: device size, persistent-grid
// size, environment switches and the operand checks of the launchers.
#pragma once
#include "rdn_common.h"

#include <stdlib.h>

// Default-on switch: off only when the variable starts with '0'.  Call sites keep it in
// a `static const bool`, so each variable is read once (knobs).
static inline bool rdn_env_on(const char* name) {
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}

// Positive integer knob: the variable's value if it is > 0, else dflt (read once, likewise)
static inline int rdn_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : dflt;
}

// CU count of the current device, cached.  A failed query or a count below 8 (one CU
// per XCD; no device this library supports reports fewer) counts as 256.
static inline int rdn_cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
    cus = n;
  }
  return cus;
}

// resident blocks per CU of one kernel instantiation (registers, LDS, waves), from the
// runtime's occupancy calculator, capped; the persistent grids are sized to it
template <typename K>
int resident_per_cu(K kernel, int threads, int cap) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0) != hipSuccess || n < 1) n = 1;
  return n < cap ? n : cap;
}

// Blocks of a persistent grid over `items` work items at `bpc` blocks per CU: a multiple
// of 8 (the kernels cut the items into one range per XCD), per XCD at most that range's
// items and at least one.  nh > 1: the kernel runs nh blocks (column parts) per slot.
static inline int rdn_persistent_grid(int64_t items, int bpc, int nh = 1) {
  const int64_t per_xcd = (items + 7) / 8;
  int slots = rdn_cu_count() * bpc / (8 * nh);
  if (slots > per_xcd) slots = (int)per_xcd;
  if (slots < 1) slots = 1;
  return 8 * nh * slots;
}

// byte offsets of a bf16 operand (pixel stride ps, plane stride pl) up to channel c_hi
// of pixel span_px, from a per-tile base, stay below the buffer descriptors' RDN_OOB
static inline bool rdn_fits32(int64_t span_px, int64_t ps, int64_t pl, int c_hi) {
  return 2 * (span_px * ps + rdn_coff(c_hi, ps, pl)) < (int64_t)RDN_OOB - 16;
}

// bf16 operand in whole units of ch channels (8: 16-byte units, 4: 8-byte units)
static inline bool rdn_aligned(int64_t ps, int64_t c0, const void* p, int ch = 8) {
  return ps % ch == 0 && c0 % ch == 0 && !((uintptr_t)p & (uintptr_t)(2 * ch - 1));
}
// input and packed weights of a bf16 conv in 16-byte units
static inline bool rdn_conv_in_aligned(const rdn_conv_desc* d) {
  return rdn_aligned(d->x_ps, d->x_c0, d->x) && !((uintptr_t)d->wp & 15) && d->kp % 8 == 0;
}

// blocks a split-K forward launch aims for (conv3_halo.hip / conv_gemm.hip split rules):
// RDN_SPLITK_TARGET blocks per CU (default 1: config 1's graph forward 1.08 -> 1.05 ms
// against 2, r06 -- an fp32 slice block is MFMA-bound, so a launch of more blocks than
// CUs ran its split conv_3 layers in ~16 us instead of ~9.  Slices cut at weight-stage
// instead of chunk granularity measured slower: 1.07 ms at 1, 1.18 at 2)
static inline int64_t rdn_splitk_target(int cus) {
  static const int per = rdn_env_int("RDN_SPLITK_TARGET", 1);
  return (int64_t)per * cus;
}
