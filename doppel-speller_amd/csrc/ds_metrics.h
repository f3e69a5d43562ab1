// Ranking and calibration metrics of a booster's margins ("Metrics"), computed where the margins
// lie: what ds_metrics.hip offers to the trainers (ds_train.hip, ds_train_batch.hip) and to its own entry points.
//
// A COLUMN is one vector of scores with the lists of its negative (label 0) and positive (label 1) rows.  The single
// trainer has one column per set (training, evaluation), the batched trainer one per model over the rows of the
// model's held-out fold.  Per column six unsigned 64-bit counters come back:
//   0 concordant   #{(p, n): key_p > key_n}          2 NaN positives      4 the log loss's fixed-point sum
//   1 ties         #{(p, n): key_p == key_n}         3 NaN negatives      5 unused
// with key = cut_key (ds_radix.h) of the float32 margin base_margin + score.  A row with a NaN margin belongs to
// neither class.  All of them are integer sums: the same for any schedule and from run to run.
#pragma once

#include "ds_launch.h"

namespace ds {

constexpr uint32_t kMetricAuc = DS_METRIC_AUC, kMetricLogloss = DS_METRIC_LOGLOSS;
constexpr int kMetricCounters = 6;
constexpr double kLoglossScale = 1048576.0;   // 2^20: the quantum of a row's term
constexpr double kLoglossCap = 2048.0;        // 2^11: a row's term saturates here (a NaN term too)

struct MetricColumn {
    const float *scores;                 // the score of every row of the matrix
    const int32_t *neg_rows, *pos_rows;  // the rows of the column with label 0 / label 1
    int32_t n_neg, n_pos;
    float base_margin;
    int32_t pad;
    double beta;                         // the weight of a negative row in the log loss
};

// One row of the weighted log loss, y * softplus(-m) + beta * (1 - y) * softplus(m) in float64 from the float32
// margin, softplus(x) = max(x, 0) + log1p(exp(-|x|)); saturated at kLoglossCap and quantised to units of 2^-20.
// Labels are 0 or 1, so one of the two products vanishes and only the other is computed: softplus(-m) for a positive
// row, beta * softplus(m) for a negative one.  For a finite margin that is the sum bit for bit (x + 0.0 = x); for an
// infinite margin on the row's own side (+inf positive, -inf negative) it is the true loss 0, where the product
// 0 * inf of the sum would be a NaN.  An infinite margin on the wrong side and a NaN margin take the cap.
__device__ inline unsigned long long logloss_term(float margin, bool positive, double beta)
{
    const double m = margin;
    const double tail = log1p(exp(-fabs(m)));
    const double loss = positive ? fmax(-m, 0.0) + tail : beta * (fmax(m, 0.0) + tail);
    const double term = fmin(loss, kLoglossCap);   // fmin: a NaN term takes the cap
    return static_cast<unsigned long long>(rint(term * kLoglossScale));
}

struct MetricScratch {   // the sort buffers of `columns` columns of n_keys keys each
    DeviceBuffer<uint32_t> keys_a, keys_b, table, state;   // state: OR[columns], AND[columns] of the columns' keys
    int64_t n_keys = 0;
    int32_t columns = 0;
    int allocate(int64_t keys, int32_t column_count);
    static int64_t bytes(int64_t keys, int32_t column_count);
};

// Enqueues on `stream` the kernels of `flags` for the columns d_columns[m], m = d_active[a] (d_active null: m = a),
// a < n_columns.  The counters of those columns (d_counters[m][kMetricCounters]) are cleared first; nothing else of
// d_counters is touched.
//   n_keys    the length to which every column's keys are padded and at which they are sorted: column a's keys lie at
//             a * n_keys of the scratch buffers.  It is the largest n_neg of the columns of this call (a smaller value
//             would cut a column short, a larger one only sorts more padding) and at most scratch.n_keys.  Ignored
//             without kMetricAuc.
//   max_pos   the largest n_pos, max_rows the largest n_neg + n_pos of those columns: they size the row grids.
//   block_cap > 0 caps the grids over rows, together with the metrics' own "max_blocks" option.
// No host sync.
int metrics_enqueue(hipStream_t stream, int compute_units, uint32_t flags, const MetricColumn *d_columns,
                    const int32_t *d_active, int32_t n_columns, int64_t n_keys, int64_t max_pos, int64_t max_rows,
                    MetricScratch &scratch, unsigned long long *d_counters, int64_t block_cap);

// counters of one column -> (concordant, ties, positives, negatives, logloss_sum, rows), -1 where `flags` lacks the metric
void metrics_row(uint32_t flags, const unsigned long long *counters, int64_t n_neg, int64_t n_pos, int64_t out[6]);

}  // namespace ds
