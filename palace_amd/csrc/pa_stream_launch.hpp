// Host side of a streaming element kernel's launch, shared by pa_nd_hex_stream.hip, pa_nd_hex_stream3.hip, pa_nd_hex_stream5.hip
// and pa_h1_hex_stream.hip.  Each kernel keeps its own policy (caps, fallback values, which switches it reads and when) as
// arguments at its call site.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "pa_internal.hpp"

namespace pa {

inline int stream_device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}

// SplitIO -> the fields {nsplit, xg0, xg1, xg_sel, yg} of a kernel's Args (the ghost buffers shifted by -nsplit, so that the
// kernel indexes them with the local dof itself); split == nullptr: nsplit = -1, one vector
template <typename Args>
void stream_set_split(Args &a, const SplitIO *split, int lsize) {
  a.nsplit = -1, a.xg0 = a.xg1 = nullptr, a.xg_sel = nullptr, a.yg = nullptr;
  if (!split) return;
  PA_REQUIRE(split->n_true >= 0 && split->n_true <= lsize, "split point outside the local vector");
  a.nsplit = split->n_true;
  a.xg0 = split->xg0 - split->n_true, a.xg1 = (split->xg1 ? split->xg1 : split->xg0) - split->n_true;
  a.xg_sel = split->sel, a.yg = split->yg - split->n_true;
}

// resident workgroups per CU the runtime reports for `kernel`, `fallback` if it does not answer
template <typename Kernel>
int stream_occupancy(Kernel kernel, int block, size_t lds, int fallback) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, lds) != hipSuccess || nb <= 0) nb = fallback;
  return nb;
}

inline int stream_env_int(const char *name) { return getenv(name) ? atoi(getenv(name)) : 0; }

// Workgroups per XCD of a kernel whose waves walk the `chunk` batches of their XCD with a fixed stride: one batch per wave
// at least, and not more workgroups than are resident (a workgroup that had to queue would run after the others and double the
// time).  honour_wgx: PALACE_AMD_STREAM_WGX caps the result (tests: many batches per wave on a small mesh).
inline int stream_wgx(int per_cu, int chunk, int waves_per_block, bool honour_wgx) {
  const int per_xcd = std::max(1, stream_device_cus() / 8) * per_cu;
  int wgx = std::max(1, std::min(per_xcd, (chunk + waves_per_block - 1) / waves_per_block));
  if (honour_wgx && getenv("PALACE_AMD_STREAM_WGX")) wgx = std::max(1, std::min(wgx, atoi(getenv("PALACE_AMD_STREAM_WGX"))));
  return wgx;
}

// the q-data of an H(curl) block has a streaming form: metric, one packed symmetric D, or both terms' packed D for curl-curl + mass
inline bool stream_qdata_ok(const SubOp &so) {
  return so.qd->metric || so.qd->ncomp == 6 || (so.qd->ncomp == 12 && so.qf == PA_QF_HDIVMASS_33);
}

}  // namespace pa
