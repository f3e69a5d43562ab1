// Launch knobs, one implementation for every stage: the option table behind each ds_*_option setter, the cap of a grid,
// and (ds_common.h) ds::compute_units.  A stage declares its Options and a table of them next to its constants, and its
// setter is one call of set_option; its launch code reads the values with get().  No result depends on an option.
#pragma once

#include <algorithm>
#include <atomic>

#include "ds_common.h"

namespace ds {

// One option: set_option accepts low..high, and 0 as well where zero_is_default.  Another thread may set an option while
// a launch reads it, so the value is an atomic.
struct Option {
    const char *name;
    int64_t low, high;        // inclusive
    int64_t initial;          // the value before any call of the setter, and the default where zero_is_default
    bool zero_is_default;     // 0 restores `initial`; otherwise 0 is a value like any other (where low admits it)
    std::atomic<int64_t> raw;

    Option(const char *name_, int64_t low_, int64_t high_, int64_t initial_, bool zero_is_default_ = false)
        : name(name_), low(low_), high(high_), initial(initial_), zero_is_default(zero_is_default_),
          raw(zero_is_default_ ? 0 : initial_)
    {
    }
    bool is_set() const { return raw.load() != 0; }
    // the effective value
    int64_t get() const { return value_or(initial); }
    // for an option whose default is its reader's (ds_forest_option("max_blocks"): every stage has a cap of its own)
    int64_t value_or(int64_t fallback) const
    {
        const int64_t value = raw.load();
        return zero_is_default && value == 0 ? fallback : value;
    }
};

// The body of a setter: DS_OK, or DS_E_ARG with "<entry>: ..." in ds_last_error() for a null name, a name that is not in
// the table or a value out of range.  Defined in ds_runtime.hip.
int set_option(const char *entry, Option *const *table, int count, const char *name, int64_t value);

template <int kCount>
int set_option(const char *entry, Option *const (&table)[kCount], const char *name, int64_t value)
{
    return set_option(entry, table, kCount, name, value);
}

// Blocks of a grid: `blocks`, limited by every cap that is positive, one at least.
inline unsigned grid_cap(int64_t blocks, int64_t cap = 0, int64_t second_cap = 0)
{
    if (cap > 0) blocks = std::min(blocks, cap);
    if (second_cap > 0) blocks = std::min(blocks, second_cap);
    return static_cast<unsigned>(std::max<int64_t>(blocks, 1));
}

}  // namespace ds
