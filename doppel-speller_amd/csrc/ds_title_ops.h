// What the two title generators share (ds_training.hip: the reference's generate_misspelled_name; ds_edits.hip: the
// generator that follows a learned profile): the codes of a transformed title, the per-(seed, purpose, index) stream and
// transform_title on codes.  Device functions only.
#pragma once

#include "ds_common.h"

namespace ds {

constexpr int kMisspellBlock = 64;            // one wave per workgroup, one lane per title
constexpr int kWorkBytes = 264;               // >= 255 + 2 insertions
constexpr uint8_t kSpaceCode = 1, kZeroCode = 28, kLastCode = 37;

// splitmix64 keyed by (seed, purpose, index), the first two outputs thrown away (include/doppel_amd.h, "training set")
struct Rng {
    uint64_t state;
    __device__ Rng(uint64_t seed, uint64_t purpose, uint64_t index)
    {
        state = seed * 0x9e3779b97f4a7c15ull + index * 0xd1342543de82ef95ull + purpose * 0xaf251af3b0f025b5ull;
        next();
        next();
    }
    __device__ uint64_t next()
    {
        uint64_t z = (state += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    __device__ int below(int n) { return static_cast<int>(__umul64hi(next(), static_cast<uint64_t>(n))); }
    __device__ uint64_t below64(uint64_t n) { return __umul64hi(next(), n); }
};

__device__ inline void erase_at(uint8_t *w, int &length, int at)
{
    for (int c = at; c < length - 1; ++c) w[c] = w[c + 1];
    --length;
}

__device__ inline void insert_at(uint8_t *w, int &length, int at, uint8_t code)
{
    for (int c = length; c > at; --c) w[c] = w[c - 1];
    w[at] = code;
    ++length;
}

// transform_title (common.py:28-38) from w into t: collapse runs of spaces, strip, cut to 255, strip, '0'-pad to 3;
// t is zero-filled to 255
__device__ inline int transform_into(const uint8_t *w, int length, uint8_t *t)
{
    int out = 0;
    for (int c = 0; c < length; ++c) {
        if (w[c] == kSpaceCode && (out == 0 || t[out - 1] == kSpaceCode)) continue;
        t[out++] = w[c];
    }
    while (out > 0 && t[out - 1] == kSpaceCode) --out;
    const int characters = out;
    if (out > DS_MAX_CHARS) out = DS_MAX_CHARS;
    while (out > 0 && t[out - 1] == kSpaceCode) --out;
    if (characters < 3) {
        const int pad = 3 - out;
        for (int c = out - 1; c >= 0; --c) t[c + pad] = t[c];
        for (int c = 0; c < pad; ++c) t[c] = kZeroCode;
        out = 3;
    }
    for (int c = out; c < DS_MAX_CHARS; ++c) t[c] = 0;
    return out;
}

// The finished rows of a block of kMisspellBlock lanes (scratch[lane] = the row of title first + lane, zero-filled to
// 255) go out as one contiguous run of n_rows * 255 bytes from first * 255, by coalesced dword stores when whole.
__device__ inline void write_title_rows(const uint8_t (*scratch)[kWorkBytes], int64_t first, int64_t n, uint8_t *out_enc)
{
    const int lane = threadIdx.x;
    const int64_t n_rows = n - first < kMisspellBlock ? n - first : kMisspellBlock;
    uint8_t *out = out_enc + first * DS_MAX_CHARS;
    if (n_rows == kMisspellBlock) {   // 16320 bytes = 4080 dwords, 4-byte aligned (first is a multiple of 64)
        for (int d = lane; d < kMisspellBlock * DS_MAX_CHARS / 4; d += kMisspellBlock) {
            uint32_t value = 0;
            for (int b = 0; b < 4; ++b) {
                const int o = 4 * d + b;
                value |= static_cast<uint32_t>(scratch[o / DS_MAX_CHARS][o % DS_MAX_CHARS]) << (8 * b);
            }
            reinterpret_cast<uint32_t *>(out)[d] = value;
        }
    } else {
        for (int o = lane; o < n_rows * DS_MAX_CHARS; o += kMisspellBlock) out[o] = scratch[o / DS_MAX_CHARS][o % DS_MAX_CHARS];
    }
}

}  // namespace ds
