// order_keys.h -- the order-preserving unsigned keys the median filter selects on (median_kernels.hip) and the radix sort orders
// (sort_kernels.hip): an element's bits as an unsigned integer whose order is the order of the values -- unsigned types as they are,
// signed integers with the sign bit flipped, floats as u ^ (sign ? ~0 : signbit).  32-bit keys for elements up to 32 bits (the bits
// above the element's stay 0), 64-bit keys for float64 / int64 / uint64.  median_elem turns a key back into the element's bits.
#pragma once
#include <stdint.h>

namespace dcp {

enum MedianKind : int { kKeyUnsigned = 0, kKeySigned = 1, kKeyFloat = 2 };

template <typename U>
struct MedianKey {
  typedef uint32_t type;
};
template <>
struct MedianKey<uint64_t> {
  typedef uint64_t type;
};

template <typename U, int KIND>
__device__ __forceinline__ typename MedianKey<U>::type median_key(U u) {
  typedef typename MedianKey<U>::type K;
  constexpr int kBits = (int)sizeof(U) * 8;
  constexpr K kSign = (K)1 << (kBits - 1), kAll = (K)(~(K)0) >> (sizeof(K) * 8 - kBits);
  const K k = (K)u;
  if constexpr (KIND == kKeySigned) return k ^ kSign;
  if constexpr (KIND == kKeyFloat) return k ^ ((k & kSign) ? kAll : kSign);
  return k;
}

template <typename U, int KIND>
__device__ __forceinline__ U median_elem(typename MedianKey<U>::type k) {
  typedef typename MedianKey<U>::type K;
  constexpr int kBits = (int)sizeof(U) * 8;
  constexpr K kSign = (K)1 << (kBits - 1), kAll = (K)(~(K)0) >> (sizeof(K) * 8 - kBits);
  if constexpr (KIND == kKeySigned) return (U)(k ^ kSign);
  if constexpr (KIND == kKeyFloat) return (U)(k ^ ((k & kSign) ? kSign : kAll));
  return (U)k;
}

}  // namespace dcp
