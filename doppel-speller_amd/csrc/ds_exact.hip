// Exact matches (Prediction._find_exact_matches, doppelspeller/predict.py:97-113) on the device.
//
// Reference: `_get_truth_data_mappings` (:74-78) builds {transformed title: title_id} by walking the truth rows in order,
// so when several rows hold the same title the LAST one wins; a query whose transformed title is a key of that dict is
// matched to it.  Here a title is its (length, code bytes) row of a ds_titles table: the encoding is injective on
// transformed titles, so equal rows <=> equal titles.
//
// The table: an open-addressing hash table of int32 truth rows (-1 = empty) with linear probing, capacity = the power of
// two >= 2N (8..16 bytes per truth row), built lazily on the first exact-match call and kept on the truth handle.
//   insert  one lane per truth row: CAS the row into the first empty slot of its probe sequence; a slot that already
//           holds the same title (compared byte by byte, never by hash alone) takes atomicMax of the two rows.  A slot's
//           title never changes once it is claimed, so every row of one title stops at the same slot and the slot ends
//           up holding the largest row of that title whatever the order in which the lanes ran.
//   probe   one lane per query: walk the probe sequence until an empty slot (absent) or a slot of the same title.
// "exact_hash_bits" (ds_titles_option) keeps only the low bits of the 64-bit title hash: tests force collisions with it.
#include "ds_launch.h"

namespace ds {

// 64-bit hash of (length, bytes): 8 bytes at a time through mix64 (ds_common.h)
__device__ inline uint64_t title_hash(const uint8_t *title, int length)
{
    uint64_t h = mix64(0x9e3779b97f4a7c15ull ^ static_cast<uint64_t>(length));
    for (int i = 0; i < length; i += 8) {
        uint64_t word = 0;
        const int end = i + 8 < length ? i + 8 : length;
        for (int j = i; j < end; ++j) word |= static_cast<uint64_t>(title[j]) << (8 * (j - i));
        h = mix64(h ^ word);
    }
    return h;
}

__device__ inline bool same_title(const uint8_t *a, int la, const uint8_t *b, int lb)
{
    if (la != lb) return false;
    for (int i = 0; i < la; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void ds_exact_insert_kernel(const uint8_t *enc, int64_t stride, const uint8_t *len,
                                                              int64_t n, uint64_t hash_mask, int32_t *slots,
                                                              uint64_t slot_mask)
{
    const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint8_t *mine = enc + row * stride;
    const int length = len[row];
    uint64_t s = title_hash(mine, length) & hash_mask & slot_mask;
    for (uint64_t step = 0; step <= slot_mask; ++step, s = (s + 1) & slot_mask) {  // the table is never full (capacity >= 2N)
        const int32_t seen = atomicCAS(&slots[s], -1, static_cast<int32_t>(row));
        if (seen == -1) return;
        if (same_title(enc + static_cast<int64_t>(seen) * stride, len[seen], mine, length)) {
            atomicMax(&slots[s], static_cast<int32_t>(row));   // predict.py:74-78: the last truth row of a title wins
            return;
        }
    }
}

__global__ __launch_bounds__(256) void ds_exact_probe_kernel(const uint8_t *t_enc, int64_t t_stride, const uint8_t *t_len,
                                                             const uint8_t *q_enc, int64_t q_stride, const uint8_t *q_len,
                                                             int64_t q_first, int64_t n, uint64_t hash_mask,
                                                             const int32_t *slots, uint64_t slot_mask, int32_t *exact_row,
                                                             int32_t *best_row)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *mine = q_enc + (q_first + i) * q_stride;
    const int length = q_len[q_first + i];
    uint64_t s = title_hash(mine, length) & hash_mask & slot_mask;
    int32_t found = -1;
    for (uint64_t step = 0; step <= slot_mask; ++step, s = (s + 1) & slot_mask) {
        const int32_t row = slots[s];
        if (row < 0) break;
        if (same_title(t_enc + static_cast<int64_t>(row) * t_stride, t_len[row], mine, length)) {
            found = row;
            break;
        }
    }
    exact_row[i] = found;
    if (best_row != nullptr && found >= 0) best_row[i] = found;   // the exact stage decides before the fuzzy one
}

static uint64_t hash_mask_of(int bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }

// The truth table's hash table, built on `stream` in front of the first probe (a caller that switches between streams
// orders them itself, as for the truth records of ds_features.hip).
static int ensure_exact_table(ds_titles *truth, hipStream_t stream)
{
    if (truth->exact_slots.ptr != nullptr) return DS_OK;
    DS_REQUIRE(truth->n <= INT32_MAX, "ds_exact_matches: more than 2^31 - 1 truth rows");
    uint64_t capacity = 16;
    while (capacity < 2 * static_cast<uint64_t>(truth->n)) capacity <<= 1;
    const size_t bytes = capacity * sizeof(int32_t);
    DS_TRY(ds::check_free(static_cast<int64_t>(bytes), "ds_exact_matches: the exact-match table"));
    DS_TRY(truth->exact_slots.allocate(static_cast<size_t>(capacity)));
    DS_HIP(hipMemsetAsync(truth->exact_slots.ptr, 0xff, bytes, stream));   // -1 = empty
    // spelled out: a failed launch releases the table, so that the next call builds it again
    hipLaunchKernelGGL(ds_exact_insert_kernel, dim3(static_cast<unsigned>((truth->n + 255) / 256)), dim3(256), 0, stream,
                       truth->enc.ptr, truth->stride, truth->len.ptr, truth->n, hash_mask_of(truth->exact_hash_bits),
                       truth->exact_slots.ptr, capacity - 1);
    const hipError_t launched = hipGetLastError();
    if (launched != hipSuccess) {
        truth->exact_slots.release();
        return ds::hip_failed(launched, "ds_exact_insert_kernel", __FILE__, __LINE__);
    }
    return DS_OK;
}

}  // namespace ds

extern "C" {

int ds_exact_matches_device(ds_titles *truth, ds_titles *queries, int64_t q_first, int64_t n_queries,
                            int32_t *d_exact_row, int32_t *d_best_row, void *stream)
{
    DS_REQUIRE(truth && queries, "ds_exact_matches: null table");
    DS_REQUIRE(queries->device == truth->device, "ds_exact_matches: tables on different devices");
    DS_REQUIRE(q_first >= 0 && n_queries >= 0 && q_first + n_queries <= queries->n,
               "ds_exact_matches: query rows [%lld, %lld) outside the table of %lld", (long long)q_first,
               (long long)(q_first + n_queries), (long long)queries->n);
    if (n_queries == 0) return DS_OK;
    DS_REQUIRE(d_exact_row != nullptr, "ds_exact_matches: null output");
    DS_HIP(hipSetDevice(truth->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DS_TRY(ds::ensure_exact_table(truth, s));
    DS_LAUNCH(ds::ds_exact_probe_kernel, dim3(static_cast<unsigned>((n_queries + 255) / 256)), dim3(256), 0, s,
              truth->enc.ptr, truth->stride, truth->len.ptr, queries->enc.ptr, queries->stride, queries->len.ptr,
              q_first, n_queries, ds::hash_mask_of(truth->exact_hash_bits), truth->exact_slots.ptr,
              static_cast<uint64_t>(truth->exact_slots.count) - 1, d_exact_row, d_best_row);
    return DS_OK;
}

int ds_exact_matches(ds_titles *truth, ds_titles *queries, int64_t n_queries, int32_t *exact_row)
{
    DS_REQUIRE(truth && queries, "ds_exact_matches: null table");
    DS_REQUIRE(n_queries >= 0 && n_queries <= queries->n, "ds_exact_matches: bad query count");
    if (n_queries == 0) return DS_OK;
    DS_REQUIRE(exact_row != nullptr, "ds_exact_matches: null output");
    DS_HIP(hipSetDevice(truth->device));
    ds::DeviceBuffer<int32_t> d_exact;
    DS_TRY(d_exact.allocate(static_cast<size_t>(n_queries)));
    DS_TRY(ds_exact_matches_device(truth, queries, 0, n_queries, d_exact.ptr, nullptr, nullptr));
    DS_HIP(hipStreamSynchronize(nullptr));
    DS_HIP(hipMemcpy(exact_row, d_exact.ptr, static_cast<size_t>(n_queries) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return DS_OK;
}

}  // extern "C"
