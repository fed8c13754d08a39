// What more than one unit of the C ABI (abi_*.hip) needs beside the key object: staging of host buffers, the scan fan-in.
#pragma once
#include "key.hpp"

// fan-in of the upper levels of the division scan (tuning hook)
inline uint32_t scan_fan() {
  static const uint32_t g = []() { const char* e = getenv("PC_HIP_SCAN_G"); int v = e ? atoi(e) : 0; return (uint32_t)(v >= 2 ? v : 16); }();
  return g;
}

// A buffer for the length of one call: the context's grow-only staging slot up to STAGE_KEEP, a transient allocation above it, freed
// when the call returns (after the context's queue has drained)
struct CallBuf {
  pc::HipBackend& be; void* dev; bool owned;
  CallBuf(pc::HipBackend& b, int slot, size_t bytes) : be(b), owned(bytes > pc::HipBackend::STAGE_KEEP) { dev = owned ? be.alloc(bytes) : be.stage(slot, bytes); }
  ~CallBuf() { if (owned) { (void)hipStreamSynchronize(be.stream); be.free(dev); } }
};

// Stage a host buffer on the device (or pass a device pointer through).
struct Staged {
  pc::HipBackend& be; void* dev = nullptr; bool owned = false;
  // slot 0 / 1: the context's grow-only staging buffers (input / output of the call); -1 or a large request: transient
  Staged(pc::HipBackend& b, const void* p, pc_mem where, size_t bytes, bool copy_in, int slot = -1) : be(b) {
    if (where == PC_MEM_DEVICE) { dev = const_cast<void*>(p); return; }
    if (slot >= 0 && bytes <= pc::HipBackend::STAGE_KEEP) dev = be.stage(slot, bytes);
    else { dev = be.alloc(bytes); owned = true; }
    if (copy_in && bytes) be.copy_h2d(dev, p, bytes);
  }
  ~Staged() { if (owned) be.free(dev); }
};

// The vectors of an opening's rounds (pc_hip_ipa_open_rounds, pc_hip_te_ipa_open_rounds): the context's grow-only buffers -- 0: the
// powers of z, 1: the per-base factors of the fixed key, 2: the two scalar vectors of its rounds.  Call inside guarded().
inline void* ipa_buffer(pc_ctx* ctx, int i, size_t bytes) {
  if (bytes > ctx->ipa_bytes[i]) {
    if (ctx->ipa_buf[i]) { ctx->be.sync(); ctx->be.free(ctx->ipa_buf[i]); ctx->ipa_buf[i] = nullptr; ctx->ipa_bytes[i] = 0; }
    ctx->ipa_buf[i] = ctx->be.alloc(bytes); ctx->ipa_bytes[i] = bytes;
  }
  return ctx->ipa_buf[i];
}

// pc_hip_shutdown's share of the Brakedown code objects (abi_lincode.hip): their device memory goes, a code its caller still holds
// stays behind as a tombstone that pc_hip_brakedown_code_free only deletes
void lincodes_shutdown(pc_ctx* ctx);
