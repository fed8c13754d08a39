// TEST-ONLY: how a probe body (probe_bodies.hpp) is run.  The same units compile twice:
//   hipcc --offload-arch=gfx950  -> tests/hip/libpc_probe.so       one device lane per index, 256-lane groups
//   g++ -x c++                   -> tests/hip/libpc_probe_host.so  the same bodies looped over on the host
// Both export the same extern "C" entry points: host pointers in and out, the return value is the HIP status (0 on the host),
// PROBE_UNSUPPORTED for an operation the field does not have (the lazy forms where LAZY_OK is false), PROBE_BAD_OP otherwise.
// Nothing here depends on the product library, its context or torch.
#pragma once
#include <stddef.h>
#include <stdint.h>

enum { PROBE_UNSUPPORTED = -1, PROBE_BAD_OP = -2 };

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace probe {

template <class Body>
__global__ void __launch_bounds__(256) k_probe(Body body, uint32_t lanes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < lanes) body(i);
}

// allocate / copy / launch / synchronise / free; buffers are sized by the caller from the case count
struct Runner {
  template <class Body>
  static int run(size_t lanes, const uint32_t* in, size_t in_words, uint32_t* out, size_t out_words, const uint32_t* aux = nullptr,
                 size_t aux_words = 0, uint32_t param = 0) {
    if (lanes == 0) return 0;
    uint32_t *din = nullptr, *dout = nullptr, *daux = nullptr;
    hipError_t e = hipMalloc((void**)&din, in_words * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, out_words * 4);
    if (e == hipSuccess && aux_words) e = hipMalloc((void**)&daux, aux_words * 4);
    if (e == hipSuccess) e = hipMemcpy(din, in, in_words * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && aux_words) e = hipMemcpy(daux, aux, aux_words * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, out_words * 4);
    if (e == hipSuccess) {
      const Body body{din, dout, daux, param};
      hipLaunchKernelGGL(k_probe<Body>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, 0, body, (uint32_t)lanes);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, out_words * 4, hipMemcpyDeviceToHost);
    (void)hipFree(din); (void)hipFree(dout); (void)hipFree(daux);
    return (int)e;
  }
};

}  // namespace probe
#else
#include <string.h>

namespace probe {

struct Runner {
  template <class Body>
  static int run(size_t lanes, const uint32_t* in, size_t, uint32_t* out, size_t out_words, const uint32_t* aux = nullptr, size_t = 0,
                 uint32_t param = 0) {
    memset(out, 0, out_words * 4);
    const Body body{in, out, aux, param};
    for (size_t i = 0; i < lanes; i++) body((uint32_t)i);
    return 0;
  }
};

}  // namespace probe
#endif

namespace probe {

// op -> Body<OP>: the operation is a template parameter of the body (one kernel per operation), chosen at run time here
template <template <int> class Body, int NOPS, int OP = 0>
int dispatch(int op, size_t n, const uint32_t* in, uint32_t* out) {
  if constexpr (OP < NOPS) {
    if (op == OP) {
      if constexpr (!Body<OP>::SUPPORTED) return PROBE_UNSUPPORTED;
      else return Runner::run<Body<OP>>(n, in, n * Body<OP>::IN_WORDS, out, n * Body<OP>::OUT_WORDS);
    }
    return dispatch<Body, NOPS, OP + 1>(op, n, in, out);
  } else {
    return PROBE_BAD_OP;
  }
}

}  // namespace probe
