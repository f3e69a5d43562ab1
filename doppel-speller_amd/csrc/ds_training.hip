// The training set of the match model on the device (FeatureEngineering.generate_train_and_evaluation_data_sets,
// doppelspeller/feature_engineering.py:172-378): the two per-row Python loops of the reference become two small kernels
// between stages that already live in HBM.
//
// Reference (doppelspeller/feature_engineering_prepare.py):
//   :25-57    get_closest_matches_per_training_row: random.sample of 10 of every train title's top-100 candidates, the
//             title's own truth row put into the sample in place of the last candidate when it is missing;
//   :60-84    EUCLIDEAN_NEIGHBOURS: the keys at distance <= 1 on a keyboard grid;
//   :90-173   generate_misspelled_name: 1 or 2 of the six edits, then transform_title (common.py:20-47).
//
// The reference draws from Python's unseeded `random`.  Here every title and every train row has a stream of its own: a
// splitmix64 sequence keyed by (seed, purpose, index) whose first two outputs are thrown away (purpose 1 = misspelling
// of truth row `index`, 2 = the sample of train row `index`); below(n) = the high 64 bits of x * n, one draw per call.
// The reference's calls map onto it as randint(a, b) = a + below(b - a + 1), choice(seq) = seq[below(len)], sample(pop,
// k) = partial Fisher-Yates.  The draws happen in the reference's order ("Training set").
//
// ds_misspell_titles: one lane per title.  A lane's working title and its scratch copy live in LDS (2 x 264 bytes per
// lane; a title grows to at most 257 characters before the cut); the block writes its finished rows (stride 255) with
// coalesced dword stores at the end.  ds_training_pairs_device: one lane per train row; the partial Fisher-Yates keeps
// only the displaced positions (at most 16) in registers, never the top_n-slot pool.
#include "ds_launch.h"
#include "ds_title_ops.h"

namespace ds {

constexpr int kMaxSample = 16;

// KEYBOARD_CARTESIAN (feature_engineering_prepare.py:14-23) per letter code 2..27 ('a'..'z'): x, y
__constant__ int8_t kKeyX[26] = {0, 4, 2, 2, 2, 3, 4, 5, 7, 6, 7, 8, 5, 5, 8, 9, 0, 3, 1, 4, 6, 3, 1, 1, 5, 0};
__constant__ int8_t kKeyY[26] = {1, 2, 2, 1, 0, 1, 1, 1, 0, 1, 1, 1, 2, 2, 0, 0, 0, 0, 1, 0, 0, 2, 0, 2, 0, 2};

__device__ inline bool near_keys(int a, int b)
{
    const int dx = kKeyX[a] - kKeyX[b], dy = kKeyY[a] - kKeyY[b];
    return a != b && dx * dx + dy * dy <= 1;
}

// random.choice(EUCLIDEAN_NEIGHBOURS[letter]) with the neighbours in ascending character order
__device__ uint8_t draw_neighbour(Rng &rng, uint8_t code)
{
    const int letter = code - 2;
    int count = 0;
    for (int b = 0; b < 26; ++b) count += near_keys(letter, b);
    int chosen = rng.below(count);
    for (int b = 0; b < 26; ++b)
        if (near_keys(letter, b) && chosen-- == 0) return static_cast<uint8_t>(b + 2);
    return code;  // not reached: every key has a neighbour
}

__device__ inline bool space_or_digit(uint8_t code) { return code == kSpaceCode || code >= kZeroCode; }

// the index of a letter the retry loops of remove_letter / add_letter / replace_letter accept (:91-99, :104-112,
// :118-126), -1 after the 11th rejected draw ("return x")
template <bool kDigitsToo>
__device__ int draw_letter(Rng &rng, const uint8_t *w, int length)
{
    int index = rng.below(length);
    for (int count = 1;; ++count) {
        const uint8_t code = w[index];
        if (!(kDigitsToo ? space_or_digit(code) : code == kSpaceCode)) return index;
        if (count > 10) return -1;
        index = rng.below(length);
    }
}

__device__ inline bool space_blocked(const uint8_t *w, int length, int index)   // :133
{
    return w[index] == kSpaceCode || w[index - 1] == kSpaceCode || index + 1 >= length || w[index + 1] == kSpaceCode;
}

// word `which` of w (split on runs of spaces): [start, end)
__device__ void find_word(const uint8_t *w, int length, int which, int &start, int &end)
{
    int position = 0;
    for (int word = 0;; ++word) {
        while (position < length && w[position] == kSpaceCode) ++position;
        start = position;
        while (position < length && w[position] != kSpaceCode) ++position;
        end = position;
        if (word == which || position >= length) return;
    }
}

enum Edit : int { kSwapWord, kAddLetter, kRemoveLetter, kReplaceLetter, kAddSpace, kRemoveSpace };

__device__ void apply_edit(Rng &rng, int edit, uint8_t *w, uint8_t *t, int &length)
{
    if (edit == kRemoveLetter) {                                              // :90-100
        const int index = draw_letter<false>(rng, w, length);
        if (index >= 0) erase_at(w, length, index);
    } else if (edit == kAddLetter) {                                          // :103-114
        const int index = draw_letter<true>(rng, w, length);
        if (index >= 0) insert_at(w, length, index, draw_neighbour(rng, w[index]));
    } else if (edit == kReplaceLetter) {                                      // :117-128
        const int index = draw_letter<true>(rng, w, length);
        if (index >= 0) w[index] = draw_neighbour(rng, w[index]);
    } else if (edit == kAddSpace) {                                           // :131-143
        int index = 1 + rng.below(length - 1);
        for (int count = 1; space_blocked(w, length, index); ++count) {
            if (count > 10) return;
            index = 1 + rng.below(length - 1);
        }
        insert_at(w, length, index, kSpaceCode);
    } else if (edit == kRemoveSpace) {                                        // :146-154
        int spaces = 0;
        for (int c = 0; c < length; ++c) spaces += w[c] == kSpaceCode;
        if (spaces == 0) return;
        int chosen = rng.below(spaces);
        for (int c = 0; c < length; ++c)
            if (w[c] == kSpaceCode && chosen-- == 0) {
                erase_at(w, length, c);
                return;
            }
    } else {                                                                  // kSwapWord, :157-162
        int words = 0;
        for (int c = 0; c < length; ++c) words += w[c] != kSpaceCode && (c == 0 || w[c - 1] == kSpaceCode);
        if (words == 0) return;   // not a transformed title (checked by the caller): nothing to swap
        const int replace = rng.below(words), other = rng.below(words);
        int position = 0, out = 0;
        for (int word = 0; word < words; ++word) {   // ' '.join(words) with the two swapped
            while (position < length && w[position] == kSpaceCode) ++position;
            int start = position;
            while (position < length && w[position] != kSpaceCode) ++position;
            int end = position;
            if (word == replace) find_word(w, length, other, start, end);
            else if (word == other) find_word(w, length, replace, start, end);
            if (word) t[out++] = kSpaceCode;
            for (int c = start; c < end; ++c) t[out++] = w[c];
        }
        for (int c = 0; c < out; ++c) w[c] = t[c];
        length = out;
    }
}

// generate_misspelled_name (:165-173) of the title in w; the result (transformed) in t
__device__ int misspell(Rng &rng, uint8_t *w, uint8_t *t, int length)
{
    const int first = rng.below(3);   // random.choice([swap_word, add_letter, remove_letter])
    const int last = rng.below(2);    // random.choice([add_space, remove_space])
    int edits[3] = {first == 0 ? kSwapWord : first == 1 ? kAddLetter : kRemoveLetter, kReplaceLetter,
                    last == 0 ? kAddSpace : kRemoveSpace};
    const int chosen = 1 + rng.below(2);   // random.randint(1, 2), then random.sample(functions, chosen)
    const int j0 = rng.below(3);
    int e0 = j0 == 0 ? edits[0] : j0 == 1 ? edits[1] : edits[2];
    if (j0 == 1) edits[1] = edits[0];
    if (j0 == 2) edits[2] = edits[0];
    int e1 = -1;
    if (chosen == 2) e1 = rng.below(2) == 0 ? edits[1] : edits[2];
    apply_edit(rng, e0, w, t, length);
    if (e1 >= 0) apply_edit(rng, e1, w, t, length);
    return transform_into(w, length, t);
}

__global__ __launch_bounds__(kMisspellBlock) void ds_misspell_kernel(
    const uint8_t *source_enc, const uint8_t *source_len, int64_t source_stride, int64_t n_source, const int32_t *rows,
    int64_t n, uint64_t seed, uint8_t *out_enc, uint8_t *out_len, int32_t *error)
{
    __shared__ uint8_t work[kMisspellBlock][kWorkBytes];
    __shared__ uint8_t scratch[kMisspellBlock][kWorkBytes];
    const int lane = threadIdx.x;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kMisspellBlock;
    const int64_t i = first + lane;
    uint8_t *w = work[lane], *t = scratch[lane];
    if (i < n) {
        const int64_t row = rows ? rows[i] : i;
        int length = 0;
        bool ok = row >= 0 && row < n_source;
        if (ok) {
            length = source_len[row];
            ok = length >= 3 && length <= DS_MAX_CHARS && length <= source_stride;
        }
        if (ok) {
            const uint8_t *title = source_enc + row * source_stride;
            bool letter = false;
            for (int c = 0; c < length; ++c) {
                const uint8_t code = title[c];
                w[c] = code;
                ok = ok && code >= kSpaceCode && code <= kLastCode;
                letter = letter || code != kSpaceCode;
            }
            ok = ok && letter;
        }
        if (ok) {
            Rng rng(seed, 1, static_cast<uint64_t>(row));
            length = misspell(rng, w, t, length);
        } else {
            atomicAdd(error, 1);
            length = 0;
            for (int c = 0; c < DS_MAX_CHARS; ++c) t[c] = 0;
        }
        out_len[i] = static_cast<uint8_t>(length);
    }
    __syncthreads();
    write_title_rows(scratch, first, n, out_enc);
}

__global__ void ds_training_pairs_kernel(const int32_t *rows, int64_t n, int32_t top_n, int32_t sample_n,
                                         const int64_t *stream_index, const int32_t *own_row, uint64_t seed,
                                         int64_t q_first, int32_t *pair_q, int32_t *pair_t, float *target)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng(seed, 2, static_cast<uint64_t>(stream_index[i]));
    // random.sample(candidates, sample_n) as partial Fisher-Yates; the pool is the identity except for the positions
    // written by earlier steps: step s records pool[key[s]] = value[s] (a later step's record wins)
    int key[kMaxSample], value[kMaxSample], candidate[kMaxSample];
#pragma unroll
    for (int s = 0; s < kMaxSample; ++s) {
        if (s < sample_n) {
            const int j = s + rng.below(top_n - s);
            int at_s = s, at_j = j;
#pragma unroll
            for (int m = 0; m < s; ++m) {
                if (key[m] == s) at_s = value[m];
                if (key[m] == j) at_j = value[m];
            }
            key[s] = j;
            value[s] = at_s;
            candidate[s] = rows[i * top_n + at_j];
        }
    }
    // :51-55: the own truth row replaces the last sampled candidate when the sample misses it
    const int32_t own = own_row[i];
    bool found = false;
#pragma unroll
    for (int s = 0; s < kMaxSample; ++s) found = found || (s < sample_n && candidate[s] == own);
    const int64_t base = (q_first + i) * sample_n;
#pragma unroll
    for (int s = 0; s < kMaxSample; ++s) {
        if (s < sample_n) {
            const int32_t row = (own >= 0 && !found && s == sample_n - 1) ? own : candidate[s];
            pair_q[base + s] = static_cast<int32_t>(q_first + i);
            pair_t[base + s] = row;
            target[base + s] = (own >= 0 && row == own) ? 1.0f : 0.0f;
        }
    }
}

}  // namespace ds

extern "C" {

int ds_misspell_titles(ds_titles *source, const int32_t *d_rows, int64_t n, uint64_t seed, void *stream, ds_titles **out)
{
    DS_REQUIRE(out != nullptr, "ds_misspell_titles: out is null");
    *out = nullptr;
    DS_REQUIRE(source != nullptr, "ds_misspell_titles: null source table");
    DS_REQUIRE(n >= 1, "ds_misspell_titles: need at least one title");
    DS_REQUIRE(n < (int64_t(1) << 31) / ds::kMisspellBlock * ds::kMisspellBlock,
               "ds_misspell_titles: too many titles");
    DS_HIP(hipSetDevice(source->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::unique_ptr<ds_titles> titles(new ds_titles());
    titles->device = source->device;
    titles->n = n;
    titles->stride = DS_MAX_CHARS;
    ds::DeviceBuffer<int32_t> error;
    DS_TRY(titles->enc.allocate(static_cast<size_t>(n) * DS_MAX_CHARS));
    DS_TRY(titles->len.allocate(static_cast<size_t>(n)));
    DS_TRY(error.allocate(1));
    int32_t errors = 0;
    DS_HIP(hipMemsetAsync(error.ptr, 0, sizeof(int32_t), s));
    DS_LAUNCH(ds::ds_misspell_kernel, dim3(static_cast<unsigned>((n + ds::kMisspellBlock - 1) / ds::kMisspellBlock)),
              dim3(ds::kMisspellBlock), 0, s, source->enc.ptr, source->len.ptr, source->stride, source->n,
              d_rows, n, seed, titles->enc.ptr, titles->len.ptr, error.ptr);
    DS_HIP(hipMemcpyAsync(&errors, error.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DS_HIP(hipStreamSynchronize(s));
    DS_REQUIRE(errors == 0, "ds_misspell_titles: %d rows are out of range or not transformed titles (3..255 codes 1..37, "
               "one letter or digit at least)", errors);
    *out = titles.release();
    return DS_OK;
}

int ds_titles_read(const ds_titles *titles, uint8_t *enc, uint8_t *len)
{
    DS_REQUIRE(titles != nullptr, "ds_titles_read: null table");
    DS_HIP(hipSetDevice(titles->device));
    if (enc) DS_HIP(hipMemcpy(enc, titles->enc.ptr, static_cast<size_t>(titles->n * titles->stride), hipMemcpyDeviceToHost));
    if (len) DS_HIP(hipMemcpy(len, titles->len.ptr, static_cast<size_t>(titles->n), hipMemcpyDeviceToHost));
    return DS_OK;
}

int ds_training_pairs_device(const int32_t *d_rows, int64_t n_queries, int32_t top_n, int32_t sample_n,
                             const int64_t *d_stream_index, const int32_t *d_own_row, uint64_t seed, int64_t q_first,
                             int32_t *d_pair_q, int32_t *d_pair_t, float *d_target, void *stream)
{
    DS_REQUIRE(n_queries >= 0 && q_first >= 0, "ds_training_pairs_device: negative query count / first query");
    DS_REQUIRE(sample_n >= 1 && sample_n <= ds::kMaxSample && sample_n <= top_n,
               "ds_training_pairs_device: need 1 <= sample_n <= min(16, top_n)");
    DS_REQUIRE((q_first + n_queries) * sample_n < (int64_t(1) << 31), "ds_training_pairs_device: too many pairs");
    if (n_queries == 0) return DS_OK;
    DS_REQUIRE(d_rows && d_stream_index && d_own_row && d_pair_q && d_pair_t && d_target,
               "ds_training_pairs_device: null pointer");
    DS_LAUNCH(ds::ds_training_pairs_kernel, dim3(static_cast<unsigned>((n_queries + 255) / 256)), dim3(256), 0,
              static_cast<hipStream_t>(stream), d_rows, n_queries, top_n, sample_n, d_stream_index, d_own_row,
              seed, q_first, d_pair_q, d_pair_t, d_target);
    return DS_OK;
}

}  // extern "C"
