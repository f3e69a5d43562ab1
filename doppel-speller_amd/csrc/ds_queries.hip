// The query side of Prediction on the device ("Query preparation"): from the raw query titles to the
// query ds_titles table (transform_title + encode_title, doppelspeller/common.py:20-47, feature_engineering.py:298-307)
// and the Jaccard query rows of a chunk of that table (the query half of the native index build, prediction.query_rows).
//
// ds_prepare_titles_kernel: one wave per title.  The raw bytes are read 64 per step, coalesced; which characters survive
// the keep filter and the ' +' -> ' ' collapse is decided from 64-bit ballots (a kept space is dropped when the previous
// kept character is a space, carried from step to step).  Only the characters after the leading strip are kept, the first
// 256 of them in an LDS row; the end of the title after the trailing strip is tracked as a position, so a title of any
// length needs no more.  The finished row is written encoded, zero-padded to 255 bytes.
//
// ds_query_rows_kernel: one wave per title.  The title's tri-grams become dense keys (37^3 of them: a transformed title
// holds 37 symbols) in LDS, ascending with the n-gram's bytes; a bitonic sort over the next power of two >= 64 orders
// them, neighbours are compared to drop repeats and the dense column table (int32[37^3], -1 = not in the truth
// vocabulary) gives the columns.  One lane adds the float64 chain in ascending n-gram order.  The counting instance
// writes the row lengths and q_maxint, one workgroup scans the lengths into rowptr, the fill instance writes the columns.
#include "ds_launch.h"
#include "ds_wave.h"

#include <algorithm>
#include <cmath>

namespace ds {

constexpr int kQueryBlock = 64;                    // one wave per workgroup, one title per wave
constexpr int kRowBytes = 256;                     // LDS row of a title being transformed (>= 255)
constexpr int kAlphabet = 37;                      // ' ', 0-9, a-z
constexpr int kDenseKeys = kAlphabet * kAlphabet * kAlphabet;
constexpr int kMaxGrams = DS_MAX_CHARS - 2;        // tri-grams of a 255-character title
constexpr int kRowptrScanThreads = 1024;
constexpr uint32_t kPadKey = 0xffffffffu;

struct PrepareReport {
    uint32_t bad[4];                 // bit b: byte b (< 128) occurs where a transformed title cannot hold it
    unsigned long long first_long;   // first title longer than 255 characters (transform = 0), else ~0
    unsigned long long first_non_ascii;
};

__device__ inline bool ascii_space(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }

__device__ inline bool kept_letter(uint32_t c) { return (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9'); }

// encode_title's code of a byte (ALLOWED_CHARACTERS = "- abc..z0..9"): ' ' 1, a-z 2..27, 0-9 28..37, anything else 0
__device__ inline uint32_t code_of(uint32_t c)
{
    if (c == ' ') return 1;
    if (c >= 'a' && c <= 'z') return c - 'a' + 2;
    if (c >= '0' && c <= '9') return c - '0' + 28;
    return 0;
}

// rank of a code in byte order (' ' < '0'..'9' < 'a'..'z'), -1 for a code that is no character of a transformed title
__host__ __device__ inline int rank_of_code(uint32_t code)
{
    if (code == 1) return 0;
    if (code >= 28 && code <= 37) return static_cast<int>(code) - 27;
    if (code >= 2 && code <= 27) return static_cast<int>(code) + 9;
    return -1;
}

__host__ inline int rank_of_byte(uint32_t c)
{
    if (c == ' ') return 0;
    if (c >= '0' && c <= '9') return static_cast<int>(c - '0') + 1;
    if (c >= 'a' && c <= 'z') return static_cast<int>(c - 'a') + 11;
    return -1;
}

__global__ __launch_bounds__(kQueryBlock) void ds_prepare_titles_kernel(const uint8_t *__restrict__ chars,
                                                                         const int64_t *__restrict__ offsets, int transform,
                                                                         uint8_t *__restrict__ enc, uint8_t *__restrict__ len,
                                                                         PrepareReport *report)
{
    __shared__ uint8_t row[kRowBytes];
    const int64_t t = blockIdx.x;
    const int lane = static_cast<int>(threadIdx.x);
    const uint64_t below = (uint64_t(1) << lane) - 1;
    // 32-bit positions throughout (ds_prepare_titles refuses titles above 2^30 bytes): this compiler lowered a
    // wave-uniform 64-bit signed compare to a vector compare and then selected on a stale scalar condition code
    const int64_t start = offsets[t];
    const int length = static_cast<int>(offsets[t + 1] - start);
    uint8_t *out = enc + t * DS_MAX_CHARS;
    uint32_t bad[4] = {0u, 0u, 0u, 0u};
    bool non_ascii = false;

    if (!transform) {  // the titles are transformed already: encode only
        for (int i = lane; i < length; i += kQueryBlock) {
            const uint32_t c = chars[start + i];
            const uint32_t code = code_of(c);
            non_ascii |= c >= 128;
            if (code == 0 && c < 128) bad[c >> 5] |= 1u << (c & 31);
            if (i < DS_MAX_CHARS) out[i] = static_cast<uint8_t>(code);
        }
        for (int i = length + lane; i < DS_MAX_CHARS; i += kQueryBlock) out[i] = 0;
        if (lane == 0) {
            len[t] = static_cast<uint8_t>(length > DS_MAX_CHARS ? DS_MAX_CHARS : length);
            if (length > DS_MAX_CHARS) atomicMin(&report->first_long, static_cast<unsigned long long>(t));
        }
    } else {
        bool carry_space = false, started = false;  // last kept character a ' '; a non-space character was written
        int written = 0, end = 0;                    // characters after the leading strip; end of the last non-space one
        for (int base = 0; base < length; base += kQueryBlock) {
            const int i = base + lane;
            uint32_t c = i < length ? chars[start + i] : 0u;
            non_ascii |= c >= 128;
            if (c >= 'A' && c <= 'Z') c += 32;                                   // lower case
            if (c == '-') c = ' ';                                               // '-' -> ' '
            const bool white = ascii_space(c);
            const bool keep = i < length && (kept_letter(c) || white);           // [a-z0-9\s]
            const uint64_t kept = __ballot(keep), spaces = __ballot(keep && c == ' ');
            const uint64_t earlier = kept & below;
            const bool after_space = earlier ? ((spaces >> (63 - __clzll(earlier))) & 1) != 0 : carry_space;
            const bool emit = keep && !(c == ' ' && after_space);                // ' +' -> ' '
            if (kept) carry_space = ((spaces >> (63 - __clzll(kept))) & 1) != 0;
            uint64_t emitted = __ballot(emit);
            const uint64_t solid = __ballot(emit && !white);
            if (!started) {
                if (!solid) continue;                                            // leading white space: stripped
                emitted &= ~((uint64_t(1) << (__ffsll(static_cast<unsigned long long>(solid)) - 1)) - 1);
                started = true;
            }
            const int at = written + __popcll(emitted & below);
            if (((emitted >> lane) & 1) && at < kRowBytes) row[at] = static_cast<uint8_t>(c);
            if (solid) {
                const int last = 63 - __clzll(solid);
                end = written + __popcll(emitted & ((uint64_t(1) << last) - 1)) + 1;
            }
            written += __popcll(emitted);
        }
        __syncthreads();
        // number_of_characters (common.py:30) = end; cut to 255 and strip again (:31), '0'-pad below 3 (:33-37)
        int body = end <= DS_MAX_CHARS ? end : 0;
        const int pad = end < 3 ? 3 - end : 0;
        if (end > DS_MAX_CHARS)
            for (int base = 0; base < DS_MAX_CHARS; base += kQueryBlock) {
                const int i = base + lane;
                const uint64_t solid = __ballot(i < DS_MAX_CHARS && !ascii_space(row[i]));
                if (solid) body = base + 64 - __clzll(solid);
            }
        const int total = pad + body;
        for (int i = lane; i < DS_MAX_CHARS; i += kQueryBlock) {
            const uint32_t c = i < pad ? '0' : (i < total ? row[i - pad] : 0u);
            const uint32_t code = i < total ? code_of(c) : 0u;
            if (i < total && code == 0) bad[c >> 5] |= 1u << (c & 31);
            out[i] = static_cast<uint8_t>(code);
        }
        if (lane == 0) len[t] = static_cast<uint8_t>(total);
    }
    if (__ballot(non_ascii) && lane == 0) atomicMin(&report->first_non_ascii, static_cast<unsigned long long>(t));
    if (__ballot(bad[0] | bad[1] | bad[2] | bad[3]))
        for (int w = 0; w < 4; ++w) {
            const uint32_t bits = wave_or(bad[w]);
            if (lane == 0 && bits) atomicOr(&report->bad[w], bits);
        }
}

// Query rows of titles [first, first + gridDim.x): kFill = false writes the row lengths to rowptr[1 + q] and q_maxint,
// kFill = true (after the scan) writes the columns from rowptr[q] on.
template <bool kFill>
__global__ __launch_bounds__(kQueryBlock) void ds_query_rows_kernel(const uint8_t *__restrict__ enc,
                                                                     const uint8_t *__restrict__ len, int64_t stride,
                                                                     int64_t first, const int32_t *__restrict__ dense,
                                                                     const float *__restrict__ idf32,
                                                                     const double *__restrict__ idf64, double max_idf,
                                                                     int unknown_counts, int64_t *__restrict__ rowptr,
                                                                     int32_t *__restrict__ cols, double *__restrict__ maxint)
{
    __shared__ uint32_t keys[256];
    __shared__ double values[kFill ? 1 : 256];
    const int64_t q = blockIdx.x;
    const int lane = static_cast<int>(threadIdx.x);
    const uint64_t below = (uint64_t(1) << lane) - 1;
    const uint8_t *title = enc + (first + q) * stride;
    const int length = len[first + q];
    const int grams = length >= 3 ? length - 2 : 0;
    int padded = kQueryBlock;
    while (padded < grams) padded <<= 1;
    for (int i = lane; i < padded; i += kQueryBlock) {
        uint32_t key = kPadKey;
        if (i < grams) {
            const uint32_t a = title[i], b = title[i + 1], c = title[i + 2];
            const int ra = rank_of_code(a), rb = rank_of_code(b), rc = rank_of_code(c);
            // a code outside the 37 (not a transformed title) is an n-gram no truth title holds, one per byte triple
            key = (ra | rb | rc) < 0 ? kDenseKeys + ((a << 16) | (b << 8) | c)
                                     : static_cast<uint32_t>((ra * kAlphabet + rb) * kAlphabet + rc);
        }
        keys[i] = key;
    }
    __syncthreads();
    if (grams > 1)
        for (int k = 2; k <= padded; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = lane; i < padded; i += kQueryBlock) {
                    const int l = i ^ j;
                    if (l > i) {
                        const uint32_t a = keys[i], b = keys[l];
                        if ((a > b) == ((i & k) == 0)) {
                            keys[i] = b;
                            keys[l] = a;
                        }
                    }
                }
                __syncthreads();
            }
    const int64_t to = kFill ? rowptr[q] : 0;
    int listed = 0, added = 0;
    for (int base = 0; base < padded; base += kQueryBlock) {
        const int i = base + lane;
        const uint32_t key = keys[i];
        const bool distinct = i < grams && (i == 0 || keys[i - 1] != key);
        const int32_t column = distinct && key < static_cast<uint32_t>(kDenseKeys) ? dense[key] : -1;
        const bool nonzero = column >= 0 ? idf32[column] != 0.f : unknown_counts != 0;  // explicit zeros vanish
        const uint64_t list = __ballot(distinct && column >= 0 && nonzero);
        const uint64_t add = __ballot(distinct && nonzero);
        if constexpr (kFill) {
            if ((list >> lane) & 1) cols[to + listed + __popcll(list & below)] = column;
        } else {
            if ((add >> lane) & 1) values[added + __popcll(add & below)] = column >= 0 ? idf64[column] : max_idf;
        }
        listed += __popcll(list);
        added += __popcll(add);
    }
    if constexpr (!kFill) {
        __syncthreads();
        if (lane == 0) {
            double sum = 0.0;  // max_intersection_possible: left to right in ascending n-gram order, no reassociation
            for (int a = 0; a < added; ++a) sum += values[a];
            maxint[q] = sum;
            rowptr[q + 1] = listed;
        }
    }
}

// rowptr[1 .. n] holds the row lengths: inclusive scan in place, rowptr[0] = 0.  One workgroup.
__global__ __launch_bounds__(kRowptrScanThreads) void ds_query_rowptr_scan_kernel(int64_t *rowptr, int64_t n)
{
    __shared__ int64_t s_waves[kRowptrScanThreads / 64];
    if (threadIdx.x == 0) rowptr[0] = 0;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += kRowptrScanThreads) {
        const int64_t i = base + threadIdx.x;
        const int64_t value = i < n ? rowptr[1 + i] : 0;
        int64_t total;
        const int64_t before = block_exclusive<kRowptrScanThreads>(value, s_waves, total);
        if (i < n) rowptr[1 + i] = carry + before + value;   // inclusive = exclusive + the lane's own value
        carry += total;
    }
}

}  // namespace ds

// The truth vocabulary in the form the query-rows kernels read.
struct ds_query_space {
    int device = 0;
    int64_t n_columns = 0;
    double max_idf = 0.0;                 // max(idf64): the value of an n-gram the truth set lacks
    bool unknown_counts = false;          // float32(max_idf) != 0: such an n-gram adds max_idf
    ds::DeviceBuffer<int32_t> dense;      // [37^3] column of every dense tri-gram key, -1 when not in the vocabulary
    ds::DeviceBuffer<float> idf32;        // [n_columns]
    ds::DeviceBuffer<double> idf64;       // [n_columns]
};

extern "C" {

int ds_query_space_create(const uint32_t *vocabulary_keys, const float *idf32, const double *idf64, int64_t V, int device,
                          ds_query_space **out)
{
    DS_REQUIRE(out != nullptr, "ds_query_space_create: out is null");
    *out = nullptr;
    DS_REQUIRE(V >= 0 && V < (int64_t(1) << 31), "ds_query_space_create: V=%lld outside 0..2^31-1", (long long)V);
    DS_REQUIRE(V == 0 || (vocabulary_keys && idf32 && idf64), "ds_query_space_create: null pointer");
    DS_REQUIRE(device >= 0, "ds_query_space_create: negative device");
    std::vector<int32_t> dense(ds::kDenseKeys, -1);
    double max_idf = 0.0;
    for (int64_t v = 0; v < V; ++v) {
        const uint32_t key = vocabulary_keys[v];
        DS_REQUIRE(key < (1u << 24) && (v == 0 || key > vocabulary_keys[v - 1]),
                   "ds_query_space_create: vocabulary keys must be strictly ascending tri-grams (key %lld)", (long long)v);
        const int a = ds::rank_of_byte(key >> 16), b = ds::rank_of_byte((key >> 8) & 0xff), c = ds::rank_of_byte(key & 0xff);
        if ((a | b | c) >= 0) dense[(a * ds::kAlphabet + b) * ds::kAlphabet + c] = static_cast<int32_t>(v);
        // np.max: NaN wins
        if (v == 0 || std::isnan(idf64[v]) || (!std::isnan(max_idf) && idf64[v] > max_idf)) max_idf = idf64[v];
    }
    DS_HIP(hipSetDevice(device));
    ds_query_space *space = new ds_query_space();
    space->device = device;
    space->n_columns = V;
    space->max_idf = max_idf;
    space->unknown_counts = static_cast<float>(max_idf) != 0.f;
    int status = space->dense.upload(dense.data(), dense.size());
    if (status == DS_OK) status = space->idf32.upload(idf32, static_cast<size_t>(V));
    if (status == DS_OK) status = space->idf64.upload(idf64, static_cast<size_t>(V));
    if (status != DS_OK) {
        delete space;
        return status;
    }
    *out = space;
    return DS_OK;
}

void ds_query_space_destroy(ds_query_space *space)
{
    if (!space) return;
    (void)hipSetDevice(space->device);
    delete space;
}

int ds_prepare_titles(const uint8_t *chars, const int64_t *offsets, int64_t n, int32_t transform, int device, void *stream,
                      ds_titles **out, int64_t report[4])
{
    DS_REQUIRE(out != nullptr && report != nullptr, "ds_prepare_titles: null out / report");
    *out = nullptr;
    report[0] = report[1] = 0;
    report[2] = report[3] = -1;
    DS_REQUIRE(n >= 1 && n < (int64_t(1) << 31), "ds_prepare_titles: n=%lld outside 1..2^31-1", (long long)n);
    DS_REQUIRE(transform == 0 || transform == 1, "ds_prepare_titles: transform must be 0 or 1");
    DS_REQUIRE(offsets != nullptr, "ds_prepare_titles: null offsets");
    DS_REQUIRE(offsets[0] == 0, "ds_prepare_titles: offsets[0] must be 0");
    for (int64_t t = 0; t < n; ++t) {
        DS_REQUIRE(offsets[t + 1] >= offsets[t], "ds_prepare_titles: bad offsets at %lld", (long long)t);
        DS_REQUIRE(offsets[t + 1] - offsets[t] <= (int64_t(1) << 30), "ds_prepare_titles: title %lld above 2^30 bytes",
                   (long long)t);
    }
    const int64_t bytes = offsets[n];
    DS_REQUIRE(bytes == 0 || chars != nullptr, "ds_prepare_titles: null chars");
    DS_REQUIRE(device >= 0, "ds_prepare_titles: negative device");
    DS_HIP(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::unique_ptr<ds_titles> titles(new ds_titles());
    titles->device = device;
    titles->n = n;
    titles->stride = DS_MAX_CHARS;
    ds::DeviceBuffer<uint8_t> d_chars;
    ds::DeviceBuffer<int64_t> d_offsets;
    ds::DeviceBuffer<ds::PrepareReport> d_report;
    DS_TRY(titles->enc.allocate(static_cast<size_t>(n) * DS_MAX_CHARS));
    DS_TRY(titles->len.allocate(static_cast<size_t>(n)));
    DS_TRY(d_chars.allocate(static_cast<size_t>(std::max<int64_t>(bytes, 1))));
    DS_TRY(d_offsets.allocate(static_cast<size_t>(n + 1)));
    DS_TRY(d_report.allocate(1));
    ds::PrepareReport host{{0u, 0u, 0u, 0u}, ~0ull, ~0ull};
    if (bytes) DS_HIP(hipMemcpyAsync(d_chars.ptr, chars, static_cast<size_t>(bytes), hipMemcpyHostToDevice, s));
    DS_HIP(hipMemcpyAsync(d_offsets.ptr, offsets, static_cast<size_t>(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    DS_HIP(hipMemcpyAsync(d_report.ptr, &host, sizeof(host), hipMemcpyHostToDevice, s));
    DS_LAUNCH(ds::ds_prepare_titles_kernel, dim3(static_cast<unsigned>(n)), dim3(ds::kQueryBlock), 0, s,
              d_chars.ptr, d_offsets.ptr, transform, titles->enc.ptr, titles->len.ptr, d_report.ptr);
    DS_HIP(hipMemcpyAsync(&host, d_report.ptr, sizeof(host), hipMemcpyDeviceToHost, s));
    DS_HIP(hipStreamSynchronize(s));
    report[0] = static_cast<int64_t>(host.bad[0] | (static_cast<uint64_t>(host.bad[1]) << 32));
    report[1] = static_cast<int64_t>(host.bad[2] | (static_cast<uint64_t>(host.bad[3]) << 32));
    report[2] = host.first_long == ~0ull ? -1 : static_cast<int64_t>(host.first_long);
    report[3] = host.first_non_ascii == ~0ull ? -1 : static_cast<int64_t>(host.first_non_ascii);
    DS_REQUIRE(report[3] < 0, "ds_prepare_titles: title %lld is not ASCII (apply the Unicode step first)", (long long)report[3]);
    DS_REQUIRE(report[2] < 0, "ds_prepare_titles: title %lld has %lld characters (stride %d)", (long long)report[2],
               (long long)(offsets[report[2] + 1] - offsets[report[2]]), DS_MAX_CHARS);
    *out = titles.release();
    return DS_OK;
}

int ds_query_rows_device(const ds_query_space *space, const ds_titles *titles, int64_t first, int64_t n,
                         int64_t *d_rowptr, int32_t *d_cols, double *d_maxint, int64_t cols_capacity, void *stream)
{
    DS_REQUIRE(space != nullptr && titles != nullptr, "ds_query_rows_device: null space / titles");
    DS_REQUIRE(first >= 0 && n >= 0 && n < (int64_t(1) << 31), "ds_query_rows_device: bad first=%lld / n=%lld",
               (long long)first, (long long)n);
    DS_REQUIRE(first + n <= titles->n, "ds_query_rows_device: titles [%lld, %lld) beyond the table's %lld",
               (long long)first, (long long)(first + n), (long long)titles->n);
    DS_REQUIRE(space->device == titles->device, "ds_query_rows_device: space and titles on different devices");
    DS_REQUIRE(titles->stride >= DS_MAX_CHARS || n == 0, "ds_query_rows_device: table stride below %d", DS_MAX_CHARS);
    DS_REQUIRE(d_rowptr != nullptr && (n == 0 || (d_cols && d_maxint)), "ds_query_rows_device: null pointer");
    DS_REQUIRE(cols_capacity >= ds::kMaxGrams * n, "ds_query_rows_device: cols_capacity=%lld below 253 * n = %lld",
               (long long)cols_capacity, (long long)(ds::kMaxGrams * n));
    DS_HIP(hipSetDevice(space->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {
        DS_HIP(hipMemsetAsync(d_rowptr, 0, sizeof(int64_t), s));
        return DS_OK;
    }
    const dim3 grid(static_cast<unsigned>(n)), block(ds::kQueryBlock);
    DS_LAUNCH(ds::ds_query_rows_kernel<false>, grid, block, 0, s, titles->enc.ptr, titles->len.ptr, titles->stride,
              first, space->dense.ptr, space->idf32.ptr, space->idf64.ptr, space->max_idf,
              static_cast<int>(space->unknown_counts), d_rowptr, d_cols, d_maxint);
    DS_LAUNCH(ds::ds_query_rowptr_scan_kernel, dim3(1), dim3(ds::kRowptrScanThreads), 0, s, d_rowptr, n);
    DS_LAUNCH(ds::ds_query_rows_kernel<true>, grid, block, 0, s, titles->enc.ptr, titles->len.ptr, titles->stride,
              first, space->dense.ptr, space->idf32.ptr, space->idf64.ptr, space->max_idf,
              static_cast<int>(space->unknown_counts), d_rowptr, d_cols, d_maxint);
    return DS_OK;
}

}  // extern "C"
