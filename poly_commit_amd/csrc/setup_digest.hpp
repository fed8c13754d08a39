// The digest of one lane of sample_generators (ipa_pc/mod.rs:302-325, hyrax/mod.rs:119-168), shared by the twisted Edwards path
// (te_setup.hpp) and the short Weierstrass one (sw_setup.hpp): Blake2s256 over name || le64(i), or name || le64(i) || le64(j) on a
// retry, as one 64-byte block.  The names keep the prefix of the unit they were written for.
#pragma once
#include "hash.hpp"

namespace pc {

static constexpr uint32_t TE_SETUP_MAX_NAME = 48;      // name || le64(i) || le64(j) is at most one 64-byte block

// The digest input of one lane.  The name is the same for every lane: the host lays it out once as the words of a zero-padded block
// and the lane ORs its two counters in behind it, at a byte offset that need not be a multiple of 4.
struct TeSetupName {
  uint32_t words[16];      // name, zero-padded
  uint32_t len;            // <= TE_SETUP_MAX_NAME
  bool set(const void* name, size_t n) {
    if (n > TE_SETUP_MAX_NAME) return false;
    for (int k = 0; k < 16; k++) words[k] = 0;
    for (size_t k = 0; k < n; k++) words[k >> 2] |= (uint32_t)((const uint8_t*)name)[k] << (8 * (k & 3));
    len = (uint32_t)n;
    return true;
  }
};

// word k of the 64-bit little-endian counter v placed at byte offset `at` of the block (0 outside its three words)
PC_HD uint32_t te_setup_le64_word(int k, uint32_t at, uint64_t v) {
  const int rel = k - (int)(at >> 2);
  const uint32_t sh = 8 * (at & 3), lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  if (rel == 0) return lo << sh;
  if (rel == 1) return sh ? (lo >> (32 - sh)) | (hi << sh) : hi;
  if (rel == 2) return sh ? hi >> (32 - sh) : 0u;
  return 0u;
}

// Blake2s256(name || le64(i)) or, with retry, Blake2s256(name || le64(i) || le64(j)): one block, final (a message of exactly 64 bytes
// is not followed by an empty block)
PC_HD void te_setup_digest(const TeSetupName& nm, uint64_t i, bool retry, uint64_t j, uint32_t* dig) {
  Blake2s256 d; d.init();
  PC_UNROLL for (int k = 0; k < 16; k++)
    d.buf[k] = nm.words[k] | te_setup_le64_word(k, nm.len, i) | (retry ? te_setup_le64_word(k, nm.len + 8, j) : 0u);
  d.t = nm.len + (retry ? 16u : 8u);
  d.compress(true);
  PC_UNROLL for (int k = 0; k < 8; k++) dig[k] = d.h[k];
}

}  // namespace pc
