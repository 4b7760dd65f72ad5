// usv_rollout_perm_math.hpp -- the minibatch order of usv_rollout_gather_perm (usv_rollout_perm.hpp): a keyed
// bijection of [0, M) computed where it is used, in place of a stored randperm, and the two-word cursor that says
// which minibatch comes next.  Plain C++ marked __host__ __device__, no HIP types, as the other *_math.hpp: the
// kernels and a stand-alone host program (tests/test_rollout_perm_math.py) run the same functions;
// tests/rollout_perm_ref.py restates them from this comment.
//
// perm_index(seed, epoch, M, p), p in [0, M), M >= 1.  M = 1 gives 0.  Otherwise
//   bits = max(2, ceil(log2 M));  a = bits / 2 (rounded down);  b = bits - a          so 2^bits < 2 M for M > 2
//   x = p;  repeat  x = E(x)  while x >= M                                             cycle walking
// E is a Feistel network on bits bits, an alternating unbalanced one: the value is (L, R) = (x >> b, x mod 2^b) with
// L of a bits and R of b bits, and round r = 0 .. 5 maps
//   (L, R) -> (R, L xor (F(R xor key_r) mod 2^width(L)))
// so the two widths swap in every round and are (a, b) again after the six; the result is (L << b) | R.  E is a
// bijection of [0, 2^bits) whatever F is, and the walk stays one of [0, M): following x -> E(x) from p < M returns to
// p, so it meets a value below M after at most 2^bits - M steps outside.  No cap: a cap would break the bijection.
//   F(v) = murmur3's 32-bit finaliser:  v ^= v >> 16;  v *= 0x85EBCA6B;  v ^= v >> 13;  v *= 0xC2B2AE35;  v ^= v >> 16
// Halves are at most 32 bits (M < 2^63), arithmetic on them is mod 2^32.
//
// The keys.  key_0 .. key_3 are the four words of Philox4x32-10 (sde_philox, usv_sde_math.hpp) with
//   key = (seed lo, seed hi),  counter = (epoch, kPermTag, 0, 0)
// and key_4, key_5 the first two words of counter (epoch, kPermTag, 1, 0).  The gSDE, CAPS and reset streams put an
// env or row number into counter words 0 and 1 (low, high): the tag in word 1 is a number no env or row has, so the
// same seed may key all of them.  The keys depend on (seed, epoch) alone, not on M or p.
//
// perm_inverse runs the rounds backwards, (L', R') -> (R' xor (F(L' xor key_r) mod 2^width(R')), L'), r = 5 .. 0, and
// walks the same way.
//
// The cursor.  Two uint32, (epoch, batch): minibatch `batch` of epoch `epoch` is positions batch B .. batch B + B - 1.
// cursor_ticked gives (epoch, batch + 1), or (epoch + 1, 0) when batch + 1 is n_batches; epoch wraps at 2^32 as
// counter_added's word does.  A batch word that is not below n_batches (only a block written by hand holds one) is
// read as 0 by the gather and by the tick alike (cursor_batch), so no position is ever >= M.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "usv_sde_math.hpp"

namespace usv {

constexpr int kPermRounds = 6;
constexpr uint32_t kPermTag = 0x5045524Du;         // "PERM": counter word 1, where the other streams have id >> 32

// The device cursor block of usv_rollout_gather_perm.  16-B aligned.
struct alignas(16) RolloutCursor {
  uint32_t epoch, batch;
  uint32_t reserved[2];
};
static_assert(sizeof(RolloutCursor) == 16, "the cursor block's layout (gym_usv_amd/rollout.py reads it)");

struct PermKeys {
  uint32_t k[kPermRounds];
};

USV_SDE_HD PermKeys perm_keys(uint64_t seed, uint32_t epoch) {
  uint32_t o0[4], o1[4];
  sde_philox(epoch, kPermTag, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o0);
  sde_philox(epoch, kPermTag, 1u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o1);
  return PermKeys{{o0[0], o0[1], o0[2], o0[3], o1[0], o1[1]}};
}

USV_SDE_HD uint32_t perm_mix(uint32_t v) {
  v ^= v >> 16;
  v *= 0x85EBCA6Bu;
  v ^= v >> 13;
  v *= 0xC2B2AE35u;
  v ^= v >> 16;
  return v;
}

// bits of the Feistel domain for M >= 2: max(2, ceil(log2 M)), at most 63.
USV_SDE_HD int perm_bits(int64_t M) {
  int bits = 2;
  while (bits < 63 && ((uint64_t)1 << bits) < (uint64_t)M) ++bits;
  return bits;
}

USV_SDE_HD uint32_t perm_mask(int w) { return (uint32_t)(((uint64_t)1 << w) - 1u); }

// E: one pass of the network over x < 2^(a + b).
USV_SDE_HD uint64_t perm_encrypt(const PermKeys& key, int a, int b, uint64_t x) {
  uint32_t L = (uint32_t)(x >> b), R = (uint32_t)x & perm_mask(b);
  int wl = a;
  for (int r = 0; r < kPermRounds; ++r) {
    const uint32_t t = L ^ (perm_mix(R ^ key.k[r]) & perm_mask(wl));
    L = R;
    R = t;
    wl = a + b - wl;                               // L now has the other width
  }
  return ((uint64_t)L << b) | R;
}

USV_SDE_HD uint64_t perm_decrypt(const PermKeys& key, int a, int b, uint64_t y) {
  uint32_t L = (uint32_t)(y >> b), R = (uint32_t)y & perm_mask(b);
  int wr = b;
  for (int r = kPermRounds - 1; r >= 0; --r) {
    const uint32_t t = R ^ (perm_mix(L ^ key.k[r]) & perm_mask(wr));
    R = L;
    L = t;
    wr = a + b - wr;
  }
  return ((uint64_t)L << b) | R;
}

// With the keys in hand (a wave derives them once for its samples).  walk, if given, gets the passes taken (>= 1).
USV_SDE_HD int64_t perm_index_keyed(const PermKeys& key, int64_t M, int64_t p, int* walk = nullptr) {
  if (walk) *walk = 0;
  if (M <= 1) return 0;
  const int bits = perm_bits(M), a = bits / 2, b = bits - a;
  uint64_t x = (uint64_t)p;
  int n = 0;
  do {
    x = perm_encrypt(key, a, b, x);
    ++n;
  } while (x >= (uint64_t)M);
  if (walk) *walk = n;
  return (int64_t)x;
}

USV_SDE_HD int64_t perm_index(uint64_t seed, uint32_t epoch, int64_t M, int64_t p, int* walk = nullptr) {
  return perm_index_keyed(perm_keys(seed, epoch), M, p, walk);
}

USV_SDE_HD int64_t perm_inverse(uint64_t seed, uint32_t epoch, int64_t M, int64_t i) {
  if (M <= 1) return 0;
  const PermKeys key = perm_keys(seed, epoch);
  const int bits = perm_bits(M), a = bits / 2, b = bits - a;
  uint64_t x = (uint64_t)i;
  do x = perm_decrypt(key, a, b, x);
  while (x >= (uint64_t)M);
  return (int64_t)x;
}

// The batch word as it is read: one that is not below n_batches counts as 0.
USV_SDE_HD uint32_t cursor_batch(uint32_t batch, uint32_t n_batches) { return batch < n_batches ? batch : 0u; }

USV_SDE_HD void cursor_ticked(uint32_t& epoch, uint32_t& batch, uint32_t n_batches) {
  const uint32_t next = cursor_batch(batch, n_batches) + 1u;
  if (next == n_batches) {
    epoch = epoch + 1u;                            // wraps at 2^32
    batch = 0u;
  } else {
    batch = next;
  }
}

}  // namespace usv
