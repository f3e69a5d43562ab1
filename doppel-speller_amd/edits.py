"""Edit scripts of title pairs and the misspelling model learned from them (this project's own; DESIGN.md section 8, "Edit
scripts and the learned misspelling model"; the rule is stated in include/doppel_amd.h).

    edit_operations(truth_titles, titles)   -> EditScripts: per pair the optimal-string-alignment distance and the script
        of match / substitute / delete / insert / transpose that turns the truth title into the observed one
    fit_misspelling_profile(truth_titles, titles, max_edits=4)   -> MisspellingProfile: what the pairs within max_edits
        edits did, counted on the device: edits per title, per-character substitution, deletion, insertion and
        transposition counts
    generate_misspelled_names(titles, seed, profile=p), FeatureEngineering(..., misspelling_profile=p)   -> titles
        misspelled after the profile instead of after the reference's hard-wired rule

The alignment of every pair runs in ds_edit_align (one wave per pair), the generator in ds_misspell_titles_profile.
"""
import ctypes

import numpy as np

from . import _lib
from .feature_engineering import ALLOWED_CHARACTERS, MAX_CHARACTERS_ALLOWED_IN_THE_TITLE, TitleTable, encode_collection

OPERATIONS = ("match", "substitute", "delete", "insert", "transpose")      # DS_EDIT_OP_*
OPS_STRIDE = 512                                                             # DS_EDIT_OPS_STRIDE
CODES = 38                                                                   # DS_EDIT_CODES
MAX_EDITS_LIMIT = 32
# the counts block (DS_EDIT_* of include/doppel_amd.h), int64 offsets
COUNTED, SKIPPED, EDITS = 0, 1, 2
SEEN = EDITS + 33
MATCH = SEEN + CODES
DELETE = MATCH + CODES
SUBSTITUTE = DELETE + CODES
INSERT = SUBSTITUTE + CODES * CODES
TRANSPOSE = INSERT + CODES * CODES
COUNTS = TRANSPOSE + CODES * CODES
MAX_COUNT = 1 << 40
RATE_SCALE = 1 << 30
FRAME_COLUMNS = ("pair", "position", "operation", "from", "to")
PROFILE_COLUMNS = ("operation", "from", "to", "count", "rate")
# KEYBOARD_CARTESIAN of the reference (feature_engineering_prepare.py:14-23), letters a..z: what its generator calls a
# neighbour is a key at Euclidean distance <= 1
_KEY_X = np.array([0, 4, 2, 2, 2, 3, 4, 5, 7, 6, 7, 8, 5, 5, 8, 9, 0, 3, 1, 4, 6, 3, 1, 1, 5, 0])
_KEY_Y = np.array([1, 2, 2, 1, 0, 1, 1, 1, 0, 1, 1, 1, 2, 2, 0, 0, 0, 0, 1, 0, 0, 2, 0, 2, 0, 2])
KEYBOARD_NEIGHBOURS = ((_KEY_X[:, None] - _KEY_X[None, :]) ** 2 + (_KEY_Y[:, None] - _KEY_Y[None, :]) ** 2 <= 1) & \
    ~np.eye(26, dtype=bool)


def _name(code):
    return "end" if code == 0 else "space" if code == 1 else ALLOWED_CHARACTERS[code]


def _max_edits(max_edits):
    if isinstance(max_edits, bool) or not isinstance(max_edits, (int, np.integer)) or not 0 <= max_edits <= MAX_EDITS_LIMIT:
        raise ValueError(f"max_edits must be an integer in 0 .. {MAX_EDITS_LIMIT}, not {max_edits!r}")
    return int(max_edits)


def validate_misspelling_profile(counts):
    """What ds_misspell_titles_profile accepts -> the block as int64[COUNTS].  A ValueError for: another shape or a dtype
    that is not integer; a count that is negative or 2^40 or more; edits[1..32] all 0 (no misspelled pair was counted); a
    count that no alignment produces (match, delete, substitute or transpose of code 0, an inserted code 0, a character
    substituted by itself); a rate of 4 events per seen character or more."""
    if isinstance(counts, MisspellingProfile):
        counts = counts.counts
    counts = np.asarray(counts)
    if counts.shape != (COUNTS,) or not np.issubdtype(counts.dtype, np.integer):
        raise ValueError(f"a misspelling profile is {COUNTS} integer counts, not {counts.dtype}{list(counts.shape)}")
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if (counts < 0).any() or (counts >= MAX_COUNT).any():
        raise ValueError("a misspelling profile's counts lie in [0, 2^40)")
    if not counts[EDITS + 1:EDITS + 33].any():
        raise ValueError("edits[1..32] are all 0: the profile holds no misspelled pair to draw a number of edits from")
    table = {name: counts[at:at + CODES * CODES].reshape(CODES, CODES)
             for name, at in (("substitute", SUBSTITUTE), ("insert", INSERT), ("transpose", TRANSPOSE))}
    if counts[MATCH] or counts[DELETE] or table["substitute"][0].any() or table["substitute"][:, 0].any() or \
            np.diagonal(table["substitute"]).any() or table["insert"][:, 0].any() or table["transpose"][0].any() or \
            table["transpose"][:, 0].any():
        raise ValueError("a count that no alignment produces is not 0 (code 0 outside an insertion's context, or a "
                         "character substituted by itself)")
    seen = counts[SEEN:SEEN + CODES]
    events = np.stack((table["substitute"].sum(axis=1), counts[DELETE:DELETE + CODES], table["transpose"].sum(axis=1),
                       table["insert"].sum(axis=1)))
    if (events[:, seen > 0] >= 4 * seen[seen > 0]).any():
        raise ValueError("a rate is 4 events per seen character or more")
    return counts


class MisspellingProfile:
    """What a set of labelled pairs did to its titles: the counts block of ds_edit_align (`counts`, int64[COUNTS]) and its
    named views: `counted`, `skipped` (pairs within / beyond max_edits), `edits` [33] (pairs by distance), `seen` [38]
    (characters of the truth side; [0] = title ends), `match` [38], `delete` [38], `substitute` [38, 38] ([truth code,
    observed code]), `insert` [38, 38] ([code in front of which, or 0 at the end; inserted code]), `transpose` [38, 38]
    ([first, second character of the truth side]).  Codes: 0 the end of a title, 1 the space, 2..27 a-z, 28..37 0-9."""

    def __init__(self, counts, max_edits=None):
        counts = np.asarray(counts)
        if counts.shape != (COUNTS,) or not np.issubdtype(counts.dtype, np.integer):
            raise ValueError(f"a misspelling profile is {COUNTS} integer counts, not {counts.dtype}{list(counts.shape)}")
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.max_edits = None if max_edits is None else _max_edits(max_edits)
        c = self.counts
        self.edits, self.seen = c[EDITS:EDITS + 33], c[SEEN:SEEN + CODES]
        self.match, self.delete = c[MATCH:MATCH + CODES], c[DELETE:DELETE + CODES]
        self.substitute = c[SUBSTITUTE:SUBSTITUTE + CODES * CODES].reshape(CODES, CODES)
        self.insert = c[INSERT:INSERT + CODES * CODES].reshape(CODES, CODES)
        self.transpose = c[TRANSPOSE:TRANSPOSE + CODES * CODES].reshape(CODES, CODES)

    counted = property(lambda self: int(self.counts[COUNTED]))
    skipped = property(lambda self: int(self.counts[SKIPPED]))

    def edits_per_title(self):
        """{distance: pairs} over the counted pairs, distances without a pair left out."""
        return {d: int(v) for d, v in enumerate(self.edits) if v}

    def operation_shares(self):
        """{"substitute", "delete", "insert", "transpose"} -> share of all edit operations (0.0 when there is none)."""
        totals = {"substitute": int(self.substitute.sum()), "delete": int(self.delete.sum()),
                  "insert": int(self.insert.sum()), "transpose": int(self.transpose.sum())}
        every = sum(totals.values())
        return {name: (value / every if every else 0.0) for name, value in totals.items()}

    def keyboard_share(self):
        """The share of letter-for-letter substitutions whose two letters are neighbours in the reference's keyboard
        table, the only substitutions its generator makes; None when no letter was substituted by a letter."""
        letters = self.substitute[2:28, 2:28]
        total = int(letters.sum())
        return int(letters[KEYBOARD_NEIGHBOURS].sum()) / total if total else None

    def rates(self):
        """The generator's integer rates (units of 2^-30 per seen character) -> {"substitute", "delete", "transpose",
        "insert"} -> int64[38]; 0 where the character was never seen."""
        seen = self.seen.astype(object)
        events = {"substitute": self.substitute.sum(axis=1), "delete": self.delete,
                  "transpose": self.transpose.sum(axis=1), "insert": self.insert.sum(axis=1)}
        return {name: np.array([0 if s == 0 else (RATE_SCALE * int(e)) // int(s) for e, s in zip(values, seen)],
                               dtype=np.int64) for name, values in events.items()}

    def frame(self, n=20):
        """The n most frequent confusions: operation, from, to, count and rate = count / seen[from] (for an insertion
        `from` is the character in front of which it stands, "end" at the end of a title; for a transposition `to` is the
        second character; the space is spelled "space")."""
        import pandas as pd
        rows = []
        for name, table in (("substitute", self.substitute), ("insert", self.insert), ("transpose", self.transpose)):
            for a, b in zip(*np.nonzero(table)):
                rows.append((name, _name(a), _name(b), int(table[a, b]), table[a, b] / max(int(self.seen[a]), 1)))
        for a in np.nonzero(self.delete)[0]:
            rows.append(("delete", _name(a), "", int(self.delete[a]), self.delete[a] / max(int(self.seen[a]), 1)))
        rows.sort(key=lambda r: (-r[3], r[0], r[1], r[2]))
        return pd.DataFrame(rows[:n], columns=list(PROFILE_COLUMNS))

    def report(self, n=10):
        """The report of examples/learn_misspellings.py as text."""
        shares = self.operation_shares()
        keyboard = self.keyboard_share()
        lines = [f"pairs counted {self.counted}, skipped {self.skipped} (more than {self.max_edits} edits)",
                 "edits per title: " + ", ".join(f"{d}: {v}" for d, v in self.edits_per_title().items()),
                 "operations: " + ", ".join(f"{name} {share:.1%}" for name, share in shares.items()),
                 "letter substitutions that are keyboard neighbours: " +
                 ("none observed" if keyboard is None else f"{keyboard:.1%}"),
                 self.frame(n).to_string(index=False)]
        return "\n".join(lines)

    def merged(self, other):
        """The profile of both sets of pairs: the sum of the two blocks."""
        if not isinstance(other, MisspellingProfile):
            raise ValueError(f"other must be a MisspellingProfile, not {type(other).__name__}")
        return MisspellingProfile(self.counts + other.counts, self.max_edits if self.max_edits == other.max_edits else None)

    def save(self, path):
        np.savez(path, counts=self.counts, max_edits=np.int64(-1 if self.max_edits is None else self.max_edits))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as stored:
            max_edits = int(stored["max_edits"])
            return cls(stored["counts"], None if max_edits < 0 else max_edits)


class EditScripts:
    """edit_operations' result: `truth_titles`, `titles` (transformed), `distance` int32[n], `ops` uint8[n, 512] (the
    script of pair i is ops[i, :lengths[i]], one of OPERATIONS per byte) and `lengths` int32[n]."""

    def __init__(self, truth_titles, titles, distance, ops, lengths):
        self.truth_titles, self.titles = truth_titles, titles
        self.distance, self.ops, self.lengths = distance, ops, lengths

    def script(self, i):
        return self.ops[i, :self.lengths[i]]

    def _steps(self, i):
        """(operation, characters of a, characters of b) per entry of pair i's script."""
        a, b = self.truth_titles[i], self.titles[i]
        at_a = at_b = 0
        for op in self.script(i):
            take_a, take_b = ((1, 1), (1, 1), (1, 0), (0, 1), (2, 2))[op]
            yield int(op), at_a, a[at_a:at_a + take_a], b[at_b:at_b + take_b]
            at_a, at_b = at_a + take_a, at_b + take_b

    def frame(self):
        """One line per operation that is not a match: pair, position in the truth title, operation, from, to."""
        import pandas as pd
        rows = [(i, at, OPERATIONS[op], a, b) for i in range(len(self.titles)) for op, at, a, b in self._steps(i) if op]
        return pd.DataFrame(rows, columns=list(FRAME_COLUMNS))

    def render(self, i):
        """Pair i as three aligned lines: the truth title, the observed title ('-' where a side has no character) and a
        marker line ('^' under every character that differs)."""
        top, bottom, marks = [], [], []
        for op, _, a, b in self._steps(i):
            width = max(len(a), len(b))
            top.append(a.ljust(width, "-"))
            bottom.append(b.ljust(width, "-"))
            marks.append((" " if op == 0 else "^") * width)
        return "\n".join(("".join(top), "".join(bottom), "".join(marks).rstrip()))


def _table(titles, transform, device, what):
    """(transformed titles, their TitleTable in HBM); every title must be a transformed title."""
    from .prediction import _CODE_OF, _pack, check_characters, transform_or_keep
    titles = transform_or_keep(titles, transform)
    for title in titles:
        if not 3 <= len(title) <= MAX_CHARACTERS_ALLOWED_IN_THE_TITLE:
            raise ValueError(f"not a transformed title (3..255 characters): {title!r}")
    chars, offsets = _pack(titles)
    check_characters(chars, offsets, what)
    enc, lengths = encode_collection(chars, offsets, _CODE_OF)
    return titles, TitleTable(enc, lengths, None, device)


def edit_option(name, value):
    """ds_edit_option, for tests: "pairs_per_group", "max_blocks" (0 = the default).  No result depends on them."""
    _lib.set_option("ds_edit_option", name, value)


def align_tables(truth, truth_rows, observed, observed_rows, n, max_edits, d_distance=None, d_ops=None,
                 d_lengths=None, d_counts=None):
    """ds_edit_align on two tables in HBM (.handle): pair p is (truth row truth_rows[p], observed row observed_rows[p]), a
    row array (a DeviceArray of int32, or None: row p).  The outputs are DeviceArrays or None."""
    _lib.check(_lib.lib().ds_edit_align(truth.handle, _lib.pointer(truth_rows), observed.handle,
                                        _lib.pointer(observed_rows), n, max_edits, _lib.pointer(d_distance),
                                        _lib.pointer(d_ops), _lib.pointer(d_lengths), _lib.pointer(d_counts)),
               "ds_edit_align")


def fit_tables(truth, truth_rows, observed, observed_rows, n, max_edits, device=0):
    """The MisspellingProfile of the pairs of align_tables; only the counts block comes back."""
    max_edits = _max_edits(max_edits)
    d_counts = _lib.DeviceArray.from_host(np.zeros(COUNTS, np.int64), device)
    try:
        align_tables(truth, truth_rows, observed, observed_rows, n, max_edits, d_counts=d_counts)
        return MisspellingProfile(d_counts.to_host(), max_edits)
    finally:
        d_counts.free()


def _pairs(truth_titles, titles, transform, device):
    truth_titles, titles = list(truth_titles), list(titles)
    if len(truth_titles) != len(titles):
        raise ValueError(f"{len(truth_titles)} truth titles but {len(titles)} titles: pair i is (truth_titles[i], titles[i])")
    if not titles:
        return [], [], None, None
    truth_titles, truth = _table(truth_titles, transform, device, "truth")
    titles, observed = _table(titles, transform, device, "the")
    return truth_titles, titles, truth, observed


def edit_operations(truth_titles, titles, transform=True, device=0):
    """What turns truth_titles[i] into titles[i], for every i -> EditScripts.  Titles are raw strings put through
    transform_titles unless transform=False."""
    truth_titles, titles, truth, observed = _pairs(truth_titles, titles, transform, device)
    n = len(titles)
    if not n:
        return EditScripts([], [], np.zeros(0, np.int32), np.zeros((0, OPS_STRIDE), np.uint8), np.zeros(0, np.int32))
    d_distance = _lib.DeviceArray((n,), np.int32, device)
    d_ops = _lib.DeviceArray((n, OPS_STRIDE), np.uint8, device)
    d_lengths = _lib.DeviceArray((n,), np.int32, device)
    try:
        align_tables(truth, None, observed, None, n, 0, d_distance, d_ops, d_lengths)
        return EditScripts(truth_titles, titles, d_distance.to_host(), d_ops.to_host(), d_lengths.to_host())
    finally:
        for array in (d_distance, d_ops, d_lengths):
            array.free()
        truth.close()
        observed.close()


def fit_misspelling_profile(truth_titles, titles, max_edits=4, transform=True, device=0):
    """The MisspellingProfile of the pairs (truth_titles[i], titles[i]): every pair is aligned on the device and those
    within max_edits edits (0 .. 32) are counted; the others (other names of the same entity, not typos) only add to
    `skipped`.  The default of 4 is twice the two single-character edits of the reference's generator."""
    max_edits = _max_edits(max_edits)
    truth_titles, titles, truth, observed = _pairs(truth_titles, titles, transform, device)
    if not titles:
        return MisspellingProfile(np.zeros(COUNTS, np.int64), max_edits)
    try:
        return fit_tables(truth, None, observed, None, len(titles), max_edits, device)
    finally:
        truth.close()
        observed.close()


def misspell_profile_table(source, rows, seed, profile, device=0):
    """ds_misspell_titles_profile -> the handle of a device table whose row i misspells row rows[i] of the table `source`
    (rows None: every row, in order) after `profile`."""
    counts = validate_misspelling_profile(profile)
    n = source.n if rows is None else int(np.asarray(rows).shape[0])
    d_rows = None if rows is None else _lib.DeviceArray.from_host(np.ascontiguousarray(rows, dtype=np.int32), device)
    d_profile = _lib.DeviceArray.from_host(counts, device)
    handle = ctypes.c_void_p()
    try:
        _lib.check(_lib.lib().ds_misspell_titles_profile(source.handle, _lib.pointer(d_rows), n, ctypes.c_uint64(seed),
                                                         d_profile.ptr, ctypes.byref(handle)),
                   "ds_misspell_titles_profile")
    finally:
        d_profile.free()
    return handle, n
