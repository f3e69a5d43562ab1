// The wave-level and workgroup-level building blocks of the device stages, in one place: reductions over the 64 lanes
// of a wave, the key of a ranked candidate, the exclusive scan of a workgroup and the two tile bodies of a stable LSD radix sort by 8-bit digits.
// Device functions only, no kernels: every translation unit may include this header.
//
// All of them work on integers, so no result depends on the order in which values are combined, and every position
// they hand out is a function of the values alone.
#pragma once

#include <type_traits>

#include "ds_common.h"

namespace ds {

// ---- reductions over the 64 lanes of a wave: the result is in every lane ---------------------------------------------
// The value of lane (this lane ^ d); a 64-bit value travels as its two halves.
template <typename T>
__device__ __forceinline__ T wave_exchange(T value, int d)
{
    static_assert(std::is_integral<T>::value && (sizeof(T) == 4 || sizeof(T) == 8), "32-bit and 64-bit integers only");
    if constexpr (sizeof(T) == 8) {
        const uint32_t low = __shfl_xor(static_cast<uint32_t>(value), d, 64);
        const uint32_t high = __shfl_xor(static_cast<uint32_t>(static_cast<uint64_t>(value) >> 32), d, 64);
        return static_cast<T>((static_cast<uint64_t>(high) << 32) | low);
    } else {
        return static_cast<T>(__shfl_xor(static_cast<uint32_t>(value), d, 64));
    }
}

template <typename T, typename Combine>
__device__ __forceinline__ T wave_reduce(T value, Combine combine)
{
    for (int d = 32; d >= 1; d >>= 1) value = combine(value, wave_exchange(value, d));
    return value;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T value)
{
    return wave_reduce(value, [](T a, T b) { return static_cast<T>(a + b); });
}
template <typename T>
__device__ __forceinline__ T wave_max(T value)
{
    return wave_reduce(value, [](T a, T b) { return b > a ? b : a; });
}
template <typename T>
__device__ __forceinline__ T wave_or(T value)
{
    return wave_reduce(value, [](T a, T b) { return static_cast<T>(a | b); });
}
template <typename T>
__device__ __forceinline__ T wave_and(T value)
{
    return wave_reduce(value, [](T a, T b) { return static_cast<T>(a & b); });
}

// ---- the key of candidate j of a list: `high` decides, the smaller j wins among equals ------------------------------------
// Distinct for distinct j and never 0 (j >= 0), so 0 can stand for "no candidate"; wave_max over the keys of a list is
// its best candidate (ds_rank.hip, ds_hard.hip).
__device__ __forceinline__ uint64_t position_key(uint32_t high, int32_t j)
{
    return (static_cast<uint64_t>(high) << 32) | static_cast<uint32_t>(~j);
}
__device__ __forceinline__ int32_t key_position(uint64_t key) { return static_cast<int32_t>(~static_cast<uint32_t>(key)); }

// ---- exclusive scan over a workgroup ---------------------------------------------------------------------------------
// Exclusive prefix of `value` over the Threads threads of the workgroup, and the total: an inclusive scan inside each
// wave by __shfl_up, the waves' totals through s_waves[Threads / 64].  ALL threads of the workgroup must call it (it
// holds two barriers); the first barrier lets a loop call it again with the same s_waves.
template <int Threads, typename T>
__device__ inline T block_exclusive(T value, T *s_waves, T &total)
{
    static_assert(Threads % 64 == 0, "whole waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inclusive = value;
    for (int offset = 1; offset < 64; offset <<= 1) {
        const T other = __shfl_up(inclusive, offset);
        if (lane >= offset) inclusive += other;
    }
    __syncthreads();   // the previous call's wave sums have been read
    if (lane == 63) s_waves[wave] = inclusive;
    __syncthreads();
    T before = 0;
    total = 0;
    for (int w = 0; w < Threads / 64; ++w) {
        const T sum = s_waves[w];
        before += w < wave ? sum : T(0);
        total += sum;
    }
    return before + inclusive - value;
}

// ---- one pass of a stable LSD radix sort by 8-bit digits: the work of a workgroup on its tile -------------------------
// The lanes of the wave that are valid and hold the same 8-bit digit as this lane (meaningless for an invalid lane).
__device__ inline unsigned long long digit_peers(uint32_t digit, bool valid)
{
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long set = __ballot(valid && bit);
        peers &= bit ? set : ~set;
    }
    return peers;
}

// s_hist[256] = the number of items of src[begin, end) with each digit; digit_of(item) is the item's digit of the pass.
// All Threads threads of the workgroup call it; s_hist is complete (a barrier has passed) when it returns.
template <int Threads, typename Item, typename Digit>
__device__ inline void radix_count_tile(const Item *src, int64_t begin, int64_t end, Digit digit_of, uint32_t *s_hist)
{
    const int lane = threadIdx.x & 63;
    for (int d = threadIdx.x; d < 256; d += Threads) s_hist[d] = 0u;
    __syncthreads();
    for (int64_t base = begin; base < end; base += Threads) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < end;
        const uint32_t digit = valid ? digit_of(src[i]) : 0u;
        const unsigned long long peers = digit_peers(digit, valid);
        if (valid && lane == __ffsll(static_cast<long long>(peers)) - 1) atomicAdd(&s_hist[digit], __popcll(peers));
    }
    __syncthreads();
}

// Stable scatter of src[begin, end) into dst[0, n), n < 2^32.  The caller has written s_next[256], the first position
// of each digit for this tile (no barrier needed after that); s_wave_count[Threads / 64][256] is scratch.  Steps of
// Threads items in order: the rank of an item among its digit's items comes from __ballot inside its wave and from
// the counts of the waves before it through LDS.  All Threads threads of the workgroup call it.
template <int Threads, typename Item, typename Digit>
__device__ inline void radix_scatter_tile(const Item *src, Item *dst, int64_t begin, int64_t end, int64_t n,
                                          Digit digit_of, uint32_t *s_next, uint32_t (*s_wave_count)[256])
{
    constexpr int kWaves = Threads / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = threadIdx.x; d < 256; d += Threads)
        for (int w = 0; w < kWaves; ++w) s_wave_count[w][d] = 0u;
    __syncthreads();
    for (int64_t base = begin; base < end; base += Threads) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < end;
        const Item item = valid ? src[i] : Item(0);
        const uint32_t digit = valid ? digit_of(item) : 0u;
        const unsigned long long peers = digit_peers(digit, valid);
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) s_wave_count[wave][digit] = __popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t position = s_next[digit] + rank;
            for (int w = 0; w < kWaves; ++w) position += w < wave ? s_wave_count[w][digit] : 0u;
            if (position < n) dst[position] = item;   // always true for counts of the same items
        }
        __syncthreads();
        for (int d = threadIdx.x; d < 256; d += Threads) {
            uint32_t sum = 0u;
            for (int w = 0; w < kWaves; ++w) {
                sum += s_wave_count[w][d];
                s_wave_count[w][d] = 0u;
            }
            s_next[d] += sum;
        }
        __syncthreads();
    }
}

}  // namespace ds
