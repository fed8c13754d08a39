// TEST-ONLY: how a kernel body of the product is run by the probe.  probe::Runner::run (probe_runner.hpp) builds a probe body from
// {in, out, aux, param}; the bodies of csrc/te.hpp have members of their own, so run_bufs() takes a list of buffers and a `make`
// that builds the body from their device copies (on the host: from the buffers themselves).  It lives beside probe_runner.hpp, not
// in it, so that the twisted Edwards units need nothing of the other units' headers but what those already had.
#pragma once
#include "probe_runner.hpp"
#if !defined(__HIPCC__)
#include <stdlib.h>
#endif

namespace probe {

// one buffer of a run_bufs() call, `words` long: `in` is copied to it (null: zero-filled), `out` receives it afterwards (null: scratch)
struct Buf { const uint32_t* in; uint32_t* out; size_t words; };
enum { MAX_BUFS = 4 };

#if defined(__HIPCC__)
// allocate / copy / launch / synchronise / copy back / free, one lane per index
template <class Make>
int run_bufs(size_t lanes, const Buf* bufs, int nbufs, Make make) {
  if (lanes == 0) return 0;
  uint32_t* d[MAX_BUFS] = {};
  hipError_t e = nbufs <= MAX_BUFS ? hipSuccess : hipErrorInvalidValue;
  for (int k = 0; k < nbufs && e == hipSuccess; k++) {
    const size_t bytes = (bufs[k].words ? bufs[k].words : 1) * 4;
    e = hipMalloc((void**)&d[k], bytes);
    if (e == hipSuccess) e = bufs[k].in ? hipMemcpy(d[k], bufs[k].in, bufs[k].words * 4, hipMemcpyHostToDevice) : hipMemset(d[k], 0, bytes);
  }
  if (e == hipSuccess) {
    const auto body = make(d);
    hipLaunchKernelGGL(k_probe<decltype(body)>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, 0, body, (uint32_t)lanes);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  for (int k = 0; k < nbufs && e == hipSuccess; k++)
    if (bufs[k].out) e = hipMemcpy(bufs[k].out, d[k], bufs[k].words * 4, hipMemcpyDeviceToHost);
  for (int k = 0; k < nbufs && k < MAX_BUFS; k++) (void)hipFree(d[k]);
  return (int)e;
}
#else
template <class Make>
int run_bufs(size_t lanes, const Buf* bufs, int nbufs, Make make) {
  if (lanes == 0) return 0;
  if (nbufs > MAX_BUFS) return PROBE_BAD_OP;
  uint32_t* d[MAX_BUFS] = {};
  for (int k = 0; k < nbufs; k++) {
    d[k] = bufs[k].out ? bufs[k].out : (uint32_t*)malloc((bufs[k].words ? bufs[k].words : 1) * 4);
    if (bufs[k].in) memcpy(d[k], bufs[k].in, bufs[k].words * 4); else memset(d[k], 0, bufs[k].words * 4);
  }
  const auto body = make(d);
  for (size_t i = 0; i < lanes; i++) body((uint32_t)i);
  for (int k = 0; k < nbufs; k++) if (!bufs[k].out) free(d[k]);
  return 0;
}
#endif

}  // namespace probe
