"""Cases placed ON the edges of the query-side kernels (tests/test_gpu_query_kernels.py), and what those tests need to know
about a case FROM ITS INPUTS ALONE: ds_prepare_titles_kernel's 64-byte steps, 256-byte LDS row and cut to 255;
ds_query_rows_kernel's sort widths (64 / 128 / 256 keys), table strides and codes outside the 37; the 1024-wide chunks of
ds_query_rowptr_scan_kernel; the wrap-around of the exact-match table's probe sequence; the NaN and tie rules of
ds_best_pairs_kernel.  tests/test_query_cases_cpu.py asserts on the CPU that the committed seeds reach every edge a GPU
test is named for.  A plain module like title_cases.py: no fixtures, no GPU.

Character codes are those of encode_title: 0 = fill, 1 = space, 2..27 = a-z, 28..37 = 0-9.
"""
import itertools
import random

import numpy as np

SYMBOLS = " 0123456789abcdefghijklmnopqrstuvwxyz"        # the 37 characters of a transformed title, in byte order
ALLOWED_CHARACTERS = "- abcdefghijklmnopqrstuvwxyz0123456789"  # code -> character (feature_engineering.py:200)
CODE_OF = np.zeros(256, dtype=np.uint8)
for _code, _character in enumerate(ALLOWED_CHARACTERS):
    CODE_OF[ord(_character)] = _code
CODE_OF[ord("-")] = 0
STEP = 64                       # raw bytes per step of ds_prepare_titles_kernel
MAX_CHARACTERS = 255
WHITE = " \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f"            # what [\s] keeps and str.strip() strips, in ASCII


def encode(titles, stride=MAX_CHARACTERS, junk=0):
    """(uint8[n, stride], uint8[n]): encode_title rows of titles of at most 255 allowed characters; the bytes behind a
    title's end hold `junk` (0 in a real table)."""
    enc = np.full((len(titles), stride), junk, dtype=np.uint8)
    lengths = np.zeros(len(titles), dtype=np.uint8)
    for row, title in enumerate(titles):
        raw = np.frombuffer(title.encode("ascii"), dtype=np.uint8)
        assert raw.shape[0] <= MAX_CHARACTERS
        enc[row, :raw.shape[0]] = CODE_OF[raw]
        lengths[row] = raw.shape[0]
    return enc, lengths


# ---- the transform catalogue ----------------------------------------------------------------------------------------

TAIL_ALPHABET = ("a", "B", "7", " ", "-", ".", "\t")
TAIL_LENGTHS = range(6)
PREFIXES = (0, 61, 125, 251)    # the tail then straddles nothing, the 64-byte step, the 128-byte step, the 255 / 256 cut


def tails():
    """Every string of length 0..5 over TAIL_ALPHABET: 19,608."""
    return ["".join(t) for n in TAIL_LENGTHS for t in itertools.product(TAIL_ALPHABET, repeat=n)]


def enumerated_titles():
    """Every tail behind a prefix of 0, 61, 125 and 251 'x', 'yz' behind it where there is a prefix: 78,432 titles."""
    all_tails = tails()
    return ["x" * p + tail + ("yz" if p else "") for p in PREFIXES for tail in all_tails]


def _white(n, shift=0):
    pool = " \t\x1c\x1d\x1e\x1f "
    return "".join(pool[(i * 5 + shift) % len(pool)] for i in range(n))


def _solid(n):
    return ("abcdefghij0123456789klmnopqrstuvwxyz" * 9)[:n]


def _thinned(total, kept, filler="."):
    """`total` raw bytes of which `kept` survive the keep filter, spread evenly between removed characters."""
    out = [filler] * total
    letters = _solid(kept)
    for i in range(kept):
        out[(i * total) // kept] = letters[i]
    return "".join(out)


def fixed_titles():
    """The fixed block: (name, title) pairs, each placed on one boundary of the transform kernel."""
    out = []
    for n in (63, 64, 65, 128, 300):
        out.append((f"white only {n}", _white(n)))
        out.append((f"spaces only {n}", " " * n))
    for m in list(range(62, 67)) + list(range(126, 131)):
        out.append((f"removed run {m}", "a " + "." * m + " b"))
    for start in (64, 128):                                      # the whole step from `start` is removed characters
        for lead in (start - 1, start - 3):
            for extra in (0, 1):
                out.append((f"removed step {start} after {lead}+{extra}",
                            "x" * lead + " " + "." * (start - lead - 1 + STEP + extra) + " b"))
    for length in (63, 64, 65, 127, 128, 129):
        for begin in (length - 2, length - 1, length):
            for run in (1, 2, 3):
                out.append((f"space run {begin}+{run}", "x" * begin + " " * run + "y"))
                out.append((f"dash run {begin}+{run}", "x" * begin + "-" * run + "y"))
    for n in (63, 64, 65, 127, 128, 129):
        out.append((f"leading spaces {n}", " " * n + "ab c"))
        out.append((f"leading white {n}", _white(n, 1) + "ab c"))
        out.append((f"leading removed {n}", "." * n + "ab c"))
    for n in (253, 254, 255, 256, 257, 258, 300):
        solid = _solid(n)
        out.append((f"solid {n}", solid))
        for at in (252, 253, 254, 255, 256):                 # kept positions 253..257, counted from 1
            if at <= n - 2:
                out.append((f"solid {n} space at {at}", solid[:at] + " " + solid[at + 1:]))
                out.append((f"solid {n} tab at {at}", solid[:at] + "\t" + solid[at + 1:]))
        out.append((f"solid {n} tabs over the cut", (solid[:251] + "\t" * 5 + solid[256:])[:n]))
        out.append((f"solid {n} white over the cut", (solid[:250] + " \t \x1f \n" + solid[257:])[:n]))
    for total in (1000, 70000):
        out.append((f"{total} bytes to 2", "a" + "." * (total - 2) + "b"))
        out.append((f"{total} bytes to 0", "." * total))
        out.append((f"{total} bytes to a b", "a" + " ." * ((total - 2) // 2) + "b"))
        out.append((f"{total} bytes to 255", _thinned(total, 255)))
        out.append((f"{total} bytes, 255 letters in space runs", _thinned(total, 255, " ")))
        out.append((f"{total} bytes to 300", _thinned(total, 300)))
        out.append((f"{total} bytes to 257", _thinned(total, 257)))
    out.append(("white inside", "a\x1cb\nc\x0bd\x0ce\rf\x1dg\x1eh\x1fi\tj"))
    out.append(("every removed byte", "".join(chr(c) for c in range(128) if chr(c) not in WHITE) * 2))
    return out


def transform_titles_catalogue():
    """The raw titles of the transform catalogue: the enumeration, then the fixed block."""
    return enumerated_titles() + [title for _, title in fixed_titles()]


_KEPT, _SPACE, _SOLID = np.zeros(256, dtype=bool), np.zeros(256, dtype=bool), np.zeros(256, dtype=bool)
for _c in range(128):
    _SOLID[_c] = chr(_c).isalnum()
    _SPACE[_c] = chr(_c) in " -"
    _KEPT[_c] = _SOLID[_c] or _SPACE[_c] or chr(_c) in WHITE


def transform_trace(title):
    """What the transform kernel meets on a raw ASCII title, from the title alone: per raw byte whether the keep filter
    keeps it, whether it is then a ' ' (after '-' -> ' '), and whether it is a solid character (a letter or a digit)."""
    raw = np.frombuffer(title.encode("ascii"), dtype=np.uint8)
    return _KEPT[raw], _SPACE[raw], _SOLID[raw]


def space_run_straddles(title, step):
    """A run of kept spaces (nothing kept between them) with one before raw offset `step` and one at or after it."""
    kept, space, _ = transform_trace(title)
    if len(title) <= step:
        return False
    before = np.nonzero(kept[:step])[0]
    after = np.nonzero(kept[step:])[0]
    return bool(before.shape[0] and after.shape[0] and space[before[-1]] and space[step + after[0]])


def empty_step_between_spaces(title, step):
    """The 64 bytes from raw offset `step` hold no kept byte, the last kept byte before them and the first behind them
    are spaces: carry_space has to survive a step with kept == 0."""
    kept, space, _ = transform_trace(title)
    if len(title) <= step + STEP or kept[step:step + STEP].any():
        return False
    before = np.nonzero(kept[:step])[0]
    after = np.nonzero(kept[step + STEP:])[0]
    return bool(before.shape[0] and after.shape[0] and space[before[-1]] and space[step + STEP + after[0]])


def first_solid_offset(title):
    _, _, solid = transform_trace(title)
    where = np.nonzero(solid)[0]
    return int(where[0]) if where.shape[0] else -1


def collapsed(title):
    """The kept characters after the ' +' collapse and both strips, before the cut (what `end` counts)."""
    import re
    text = title.lower().replace("-", " ")
    text = "".join(re.findall(r"[a-z0-9\s]", text))
    return re.sub(r" +", " ", text).strip()


# ---- the query-rows catalogue ---------------------------------------------------------------------------------------

ROUNDS = 3                      # the 256 lengths x 5 styles, three times with other letters and seeds: 3,840 titles
STYLES = ("one letter", "period 2", "period 3", "random", "distinct")
CALL_COUNTS = (1, 1023, 1024, 1025, 2048, 2049, 3073)


def _distinct_string(rng):
    """255 symbols whose 253 tri-grams are all different: every prefix of it has distinct tri-grams too."""
    text = list("qqq ")                                          # the truth set's two zero-idf tri-grams lead it
    seen = {("q", "q", "q"), ("q", "q", " ")}
    while len(text) < MAX_CHARACTERS:
        choices = [c for c in SYMBOLS if (text[-2], text[-1], c) not in seen]
        c = rng.choice(choices)
        seen.add((text[-2], text[-1], c))
        text.append(c)
    return "".join(text)


def rows_titles():
    """(titles, style of each, round of each): every length 0..255 in the five styles, ROUNDS times, in a seeded order so
    that every chunk of a call holds every length."""
    titles, styles = [], []
    for r in range(ROUNDS):
        rng = random.Random(100 + r)
        one = ("qa 9z", "z0q a", "  q7m")[r]
        two = ("ab", "q ", "0z")[r]
        three = ("abc", "qqa", " 9 ")[r]
        distinct = _distinct_string(rng)
        for length in range(MAX_CHARACTERS + 1):
            titles.append(one[length % 5] * length)
            titles.append((two * 128)[:length])
            titles.append((three * 86)[:length])
            titles.append("".join(rng.choice(SYMBOLS) for _ in range(length)))
            titles.append(distinct[:length])
            styles += list(STYLES)
    order = np.random.RandomState(7).permutation(len(titles))
    return [titles[i] for i in order], [styles[i] for i in order]


def truth_titles(count=3000, seed=12):
    """Synthetic truth titles that fix the vocabulary: words of a seeded pool behind 'qqq ', so 'qqq' and 'qq ' are in
    every title (idf 0), the pool's tri-grams are known and most others are not."""
    rng = random.Random(seed)
    letters = "aaabbcdeeefghiijklmnooprsstuuy0127"
    pool = ["".join(rng.choice(letters) for _ in range(rng.randint(2, 8))) for _ in range(600)] + ["ab", "abc", "bca", "cab"]
    return ["qqq " + " ".join(rng.choice(pool) for _ in range(rng.randint(1, 6))) for _ in range(count)]


def vocabulary(truth):
    """(vocabulary_keys uint32, idf32, idf64) of the truth titles by the native index build (host code of the library)."""
    from doppel_speller_amd import prediction
    from doppel_speller_amd.match_maker import NativeProblem
    chars, offsets = prediction._pack(truth)
    problem = NativeProblem.from_flat(chars, offsets, np.zeros(1, np.uint8), np.zeros(1, np.int64), 3)
    a = problem.arrays()
    problem.close()
    return a["vocabulary_keys"], a["idf32"], a["idf64"]


def chunks(n_titles):
    """(first, n) of every ds_query_rows_device call: each count with first = 0 and with the chunk ending at the table's
    end (first > 0), and two empty chunks."""
    out = []
    for n in CALL_COUNTS:
        assert n < n_titles
        out += [(0, n), (n_titles - n, n)]
    return out + [(n_titles, 0), (n_titles // 2, 0)]


def gram_counts(lengths):
    return np.maximum(np.asarray(lengths, dtype=np.int64) - 2, 0)


def distinct_grams(title):
    return len({title[i:i + 3] for i in range(len(title) - 2)})


def invalid_code_rows(seed=31):
    """(uint8[n, 255], uint8[n]): a small table with the codes 0, 38, 64 and 255 mixed into valid ones, at the lengths where
    the sort width changes, with repeated invalid triples, whole rows of one invalid code, and invalid codes at both ends."""
    rng = np.random.RandomState(seed)
    bad = np.array([0, 38, 64, 255], dtype=np.uint8)
    rows = []
    for length in (3, 4, 5, 10, 65, 66, 67, 129, 130, 131, 200, 254, 255):
        for share in (0.02, 0.2, 0.7):
            row = rng.randint(1, 38, length).astype(np.uint8)
            hit = rng.rand(length) < share
            hit[rng.randint(length)] = True
            row[hit] = bad[rng.randint(0, 4, int(hit.sum()))]
            rows.append(row)
        row = rng.randint(1, 6, length).astype(np.uint8)         # few symbols: repeats among valid and invalid triples
        row[::3] = bad[rng.randint(0, 4)]
        rows.append(row)
        rows.append(np.full(length, bad[rng.randint(0, 4)], dtype=np.uint8))
        row = rng.randint(1, 38, length).astype(np.uint8)
        row[0], row[-1] = 255, 0
        rows.append(row)
    rows += [np.zeros(0, np.uint8), np.array([255], np.uint8), np.array([38, 0], np.uint8)]
    enc = np.zeros((len(rows), MAX_CHARACTERS), dtype=np.uint8)
    lengths = np.zeros(len(rows), dtype=np.uint8)
    for r, row in enumerate(rows):
        enc[r, :row.shape[0]] = row
        lengths[r] = row.shape[0]
    return enc, lengths


def rule_rows(enc, lengths, vocabulary_keys, idf32, idf64):
    """The rule ds_query_rows_kernel documents, in plain Python over code rows: per title the distinct code triples; the
    valid ones (all three codes among the 37) in ascending n-gram order, looked up in the vocabulary (a known one is
    listed and adds its idf64 where its idf32 is not 0, an unknown one adds max(idf64) where float32 of that is not 0);
    then every invalid triple, an unknown n-gram of its own.  The float64 sum runs left to right in that order.
    -> (rowptr int64[n + 1], cols int32, maxint float64[n])."""
    column_of = {int(key): column for column, key in enumerate(np.asarray(vocabulary_keys).tolist())}
    idf32, idf64 = np.asarray(idf32), np.asarray(idf64)
    max_idf = float(np.max(idf64)) if idf64.shape[0] else 0.0
    unknown_counts = bool(np.float32(max_idf) != 0)
    rowptr, cols, maxint = [0], [], []
    for row, length in zip(np.asarray(enc), np.asarray(lengths).tolist()):
        codes = row[:length].tolist()
        triples = {tuple(codes[i:i + 3]) for i in range(length - 2)}
        valid = [t for t in triples if all(1 <= c <= 37 for c in t)]
        invalid = sorted(t for t in triples if not all(1 <= c <= 37 for c in t))
        keyed = sorted((ord(ALLOWED_CHARACTERS[a]) << 16) | (ord(ALLOWED_CHARACTERS[b]) << 8) | ord(ALLOWED_CHARACTERS[c])
                       for a, b, c in valid)
        total = 0.0
        for key in keyed:
            column = column_of.get(key)
            if column is None:
                if unknown_counts:
                    total += max_idf
            elif idf32[column] != 0:
                cols.append(column)
                total += float(idf64[column])
        for _ in invalid:
            if unknown_counts:
                total += max_idf
        rowptr.append(len(cols))
        maxint.append(total)
    return np.array(rowptr, dtype=np.int64), np.array(cols, dtype=np.int32), np.array(maxint, dtype=np.float64)


def slice_rows(rowptr, cols, maxint, first, n):
    """The rows [first, first + n) of a CSR as a call on that chunk returns them: rowptr starts at 0."""
    lo, hi = int(rowptr[first]), int(rowptr[first + n])
    return rowptr[first:first + n + 1] - lo, cols[lo:hi], maxint[first:first + n]


# ---- exact matches --------------------------------------------------------------------------------------------------

_M64 = (1 << 64) - 1
LONG_TITLE = ("lorem ipsum dolor sit amet " * 10)[:MAX_CHARACTERS]


def exact_mix(x):
    """ds_exact.hip exact_mix (the splitmix64 finaliser), restated."""
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & _M64
    x ^= x >> 31
    return x


def title_hash(codes):
    """ds_exact.hip title_hash over the code bytes of a title, restated: the length, then 8 bytes at a time, low byte first."""
    codes = bytes(codes)
    h = exact_mix(0x9e3779b97f4a7c15 ^ len(codes))
    for i in range(0, len(codes), 8):
        h = exact_mix(h ^ int.from_bytes(codes[i:i + 8], "little"))
    return h


def capacity_of(n_rows):
    capacity = 16
    while capacity < 2 * n_rows:
        capacity <<= 1
    return capacity


def chains_past_the_end(truth, hash_bits=64):
    """How many distinct truth titles are placed by a probe sequence that passes the last slot of the table, by the
    restated hash and linear probing.  The slots a set of keys occupies, and how many placements cross a given slot
    boundary, do not depend on the order of insertion, so this holds for the device's build whatever its schedule."""
    capacity = capacity_of(len(truth))
    mask = _M64 if hash_bits >= 64 else (1 << hash_bits) - 1
    taken = [False] * capacity
    wrapped = 0
    for title in dict.fromkeys(truth):
        s = title_hash(CODE_OF[np.frombuffer(title.encode("ascii"), dtype=np.uint8)].tobytes()) & mask & (capacity - 1)
        passed = False
        while taken[s]:
            passed |= s == capacity - 1
            s = (s + 1) & (capacity - 1)
        taken[s] = True
        wrapped += passed
    return wrapped


def _distinct_titles(rng, count, letters, low=3, high=6):
    seen = {}
    while len(seen) < count:
        seen["".join(rng.choice(letters) for _ in range(rng.randint(low, high)))] = None
    return list(seen)


def exact_queries(truth, rng):
    """Every truth title, every strict prefix of it (the empty one too), every one-symbol extension of it, and a few
    absent titles; duplicates dropped, order kept."""
    queries = []
    for title in dict.fromkeys(truth):
        queries.append(title)
        queries += [title[:n] for n in range(len(title))]
        if len(title) < MAX_CHARACTERS:
            queries += [title + c for c in SYMBOLS]
    queries += ["".join(rng.choice(SYMBOLS[1:]) for _ in range(rng.randint(3, 12))) for _ in range(6)]
    queries += ["zzzzzzz", "absent title", "0"]
    return list(dict.fromkeys(queries))


def exact_tables(seed=5):
    """[(name, truth titles, queries)]: 200 tables of 8 titles (capacity 16 = 2N), one of 1,024 (capacity 2,048 = 2N), one
    with titles below three characters, a 255-character one, and later duplicates of each."""
    rng = random.Random(seed)
    tables = []
    for t in range(200):
        truth = _distinct_titles(rng, 8, "abcdefgh")
        tables.append((f"small {t}", truth, exact_queries(truth, rng)))
    # a seed of its own, one at which chains of the 1,024-title table pass slot 2,047 (tests/test_query_cases_cpu.py)
    truth = _distinct_titles(random.Random(34), 1024, "abcdefghij")
    tables.append(("1024", truth, exact_queries(truth, rng)))
    short = ["", "a", "ab", "abc", LONG_TITLE]
    truth = short + ["xyz"] + short + ["abd", ""]
    tables.append(("short and long", truth, list(dict.fromkeys(exact_queries(truth, rng) + [LONG_TITLE[:254] + "z"]))))
    return tables


def exact_expected(truth, queries):
    """predict.py:74-78: a dict filled in truth order, the last row of a title wins; -1 for an absent title."""
    last = {}
    for row, title in enumerate(truth):
        last[title] = row
    return np.array([last.get(q, -1) for q in queries], dtype=np.int32)


# ---- best pairs -----------------------------------------------------------------------------------------------------

POOL = np.array([0.0, -0.0, 0.25, 0.9, 1.0, np.inf, -np.inf, np.nan, -1.0], dtype=np.float32)
BEST_KS = (1, 2, 7, 100)
SITUATIONS = ("all equal", "all nan", "nan first then larger", "nan later only", "maximum last", "zero then minus zero",
              "minus zero then zero")


def named_rows(k):
    """{situation: float32[k]} for the situations a row of k slots can hold (k = 1: the first two only)."""
    nan = np.float32(np.nan)
    out = {"all equal": np.full(k, 0.9, np.float32), "all nan": np.full(k, nan, np.float32)}
    if k >= 2:
        row = np.full(k, 0.25, np.float32)
        row[0], row[-1] = nan, np.inf
        out["nan first then larger"] = row
        row = np.full(k, 0.25, np.float32)
        row[k // 2:] = nan
        out["nan later only"] = row
        row = np.full(k, 0.25, np.float32)
        row[-1] = 1.0
        out["maximum last"] = row
        row = np.full(k, -1.0, np.float32)
        row[0], row[-1] = 0.0, -0.0
        out["zero then minus zero"] = row
        row = np.full(k, -np.inf, np.float32)
        row[0], row[-1] = -0.0, 0.0
        out["minus zero then zero"] = row
    return out


def situation_of(row):
    """The situations (by name) a probability row is in, from the row alone."""
    row = np.asarray(row, dtype=np.float32)
    k, nan = row.shape[0], np.isnan(row)
    found = set()
    if not nan.any() and (row == row[0]).all() and row[0] != 0:
        found.add("all equal")
    if nan.all():
        found.add("all nan")
    if k >= 2:
        if nan[0] and not nan[1:].all():
            found.add("nan first then larger")
        if not nan[0] and nan[1:].any():
            found.add("nan later only")
        if not nan.any() and row[-1] > row[:-1].max():
            found.add("maximum last")
        top = np.nanmax(row) if not nan.all() else None
        if top == 0 and not nan[0]:
            zeros = np.nonzero(row == 0)[0]
            signs = np.signbit(row[zeros])
            if zeros.shape[0] >= 2 and not signs[0] and signs[1:].any():
                found.add("zero then minus zero")
            if zeros.shape[0] >= 2 and signs[0] and not signs[1:].all():
                found.add("minus zero then zero")
    return found


def best_pair_case(n_queries, k, seed):
    """(rows int32[n, k] -- any int32, negative ones too --, probabilities float32[n, k]): the named situations first (as
    many as n holds), then rows drawn from POOL, every fifth of them from a pool of two values (ties everywhere)."""
    rng = np.random.RandomState(seed)
    rows = rng.randint(-2 ** 31, 2 ** 31, (n_queries, k), dtype=np.int64).astype(np.int32)
    probabilities = POOL[rng.randint(0, POOL.shape[0], (n_queries, k))]
    few = np.arange(n_queries) % 5 == 0
    picks = POOL[rng.randint(0, POOL.shape[0], (n_queries, 2))]
    two = np.where(rng.rand(n_queries, k) < 0.5, picks[:, :1], picks[:, 1:])
    probabilities[few] = two[few]
    for q, row in enumerate(list(named_rows(k).values())[:n_queries]):
        probabilities[q] = row
    return rows, np.ascontiguousarray(probabilities, dtype=np.float32)


def best_pairs_loop(rows, probabilities):
    """The loop of the header comment, literally, one query at a time: start from slot 0, replace on `>` only, count
    `==`.  -> (pair int64, row int32, probability bits uint32, count int32)."""
    n, k = probabilities.shape
    pair, row = np.zeros(n, np.int64), np.zeros(n, np.int32)
    bits, count = np.zeros(n, np.uint32), np.zeros(n, np.int32)
    for q in range(n):
        best, where, held = probabilities[q, 0], 0, 1
        for j in range(1, k):
            p = probabilities[q, j]
            if p > best:
                best, where, held = p, j, 1
            elif p == best:
                held += 1
        pair[q], row[q], count[q] = q * k + where, rows[q, where], held
        bits[q] = np.float32(best).view(np.uint32)
    return pair, row, bits, count


def best_pairs(rows, probabilities):
    """The same loop with all queries side by side (one pass per slot), for the counts a Python loop is too slow for;
    tests/test_query_cases_cpu.py holds it against `best_pairs_loop`."""
    n, k = probabilities.shape
    best = probabilities[:, 0].copy()
    where = np.zeros(n, dtype=np.int64)
    count = np.ones(n, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for j in range(1, k):
            p = probabilities[:, j]
            larger = p > best
            count = np.where(larger, 1, count + (~larger & (p == best))).astype(np.int32)
            best = np.where(larger, p, best)
            where = np.where(larger, j, where)
    q = np.arange(n, dtype=np.int64)
    return q * k + where, rows[q, where], best.view(np.uint32), count
