"""CPU restatement of the training-set generation (FeatureEngineering.generate_train_and_evaluation_data_sets,
doppelspeller/feature_engineering.py:172-378 and feature_engineering_prepare.py) in the port's own terms: titles as
character codes (space 1, a-z 2..27, 0-9 28..37) and the per-(seed, purpose, index) splitmix64 stream that replaces
the reference's unseeded `random` ("Training set").

Plain Python / NumPy, one title or one train row at a time: the yardstick of csrc/ds_training.hip and of
doppel-speller_amd/training_set.py.  Citations are to the reference files named above.
"""
import numpy as np

MASK = (1 << 64) - 1
SPACE, FIRST_LETTER, LAST_LETTER, ZERO_DIGIT = 1, 2, 27, 28
MAX_CHARACTERS = 255                     # settings.py:68
N_GRAMS = 3                              # settings.py:15
PURPOSE_MISSPELL, PURPOSE_SAMPLE = 1, 2
KIND_GENERATED, KIND_NEGATIVE, KIND_POSITIVE = 1, 2, 3   # constants.py:46-48
ALPHABET = "- abcdefghijklmnopqrstuvwxyz0123456789"       # feature_engineering.py:200
# feature_engineering_prepare.py:14-23, letter -> (x, y)
KEYBOARD = {
    'q': (0, 0), 'w': (1, 0), 'e': (2, 0), 'r': (3, 0), 't': (4, 0), 'y': (5, 0), 'u': (6, 0), 'i': (7, 0),
    'o': (8, 0), 'p': (9, 0), 'a': (0, 1), 'z': (0, 2), 's': (1, 1), 'x': (1, 2), 'd': (2, 1), 'c': (2, 2),
    'f': (3, 1), 'b': (4, 2), 'm': (5, 2), 'j': (6, 1), 'g': (4, 1), 'h': (5, 1), 'k': (7, 1), 'l': (8, 1),
    'v': (3, 2), 'n': (5, 2),
}


class Stream:
    """splitmix64 keyed by (seed, purpose, index), the first two outputs thrown away (csrc/ds_synth.cpp `Stream`)."""

    def __init__(self, seed, purpose, index):
        self.state = (seed * 0x9e3779b97f4a7c15 + index * 0xd1342543de82ef95 + purpose * 0xaf251af3b0f025b5) & MASK
        self.next()
        self.next()

    def next(self):
        self.state = (self.state + 0x9e3779b97f4a7c15) & MASK
        z = self.state
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
        return z ^ (z >> 31)

    def below(self, n):
        """One draw in [0, n): the high 64 bits of x * n."""
        return (self.next() * n) >> 64

    # the reference's calls (random.randint / choice / sample) mapped onto the stream
    def randint(self, a, b):
        return a + self.below(b - a + 1)

    def choice(self, sequence):
        return sequence[self.below(len(sequence))]

    def sample(self, population, k):
        """Partial Fisher-Yates: pool[:k] after swapping pool[i] with pool[i + below(n - i)] for i < k."""
        pool = list(population)
        n = len(pool)
        for i in range(k):
            j = i + self.below(n - i)
            pool[i], pool[j] = pool[j], pool[i]
        return pool[:k]


def neighbour_table():
    """EUCLIDEAN_NEIGHBOURS (feature_engineering_prepare.py:60-84) as codes: code -> ascending list of codes of the
    keys at distance <= 1 (m and n share a coordinate: neighbours of each other)."""
    table = {}
    for a, (xa, ya) in KEYBOARD.items():
        near = [b for b, (xb, yb) in KEYBOARD.items() if b != a and (xa - xb) ** 2 + (ya - yb) ** 2 <= 1]
        table[ALPHABET.index(a)] = sorted(ALPHABET.index(b) for b in near)
    return table


NEIGHBOURS = neighbour_table()


def to_codes(title):
    return [ALPHABET.index(ch) for ch in title]


def to_text(codes):
    return "".join(ALPHABET[c] for c in codes)


def _is_space_or_digit(code):
    return code == SPACE or code >= ZERO_DIGIT


# ---- the six operations (feature_engineering_prepare.py:90-162), on lists of codes ------------------------------------
def remove_letter(rng, x):                                                     # :90-100
    length = len(x)
    index = rng.randint(0, length - 1)
    count = 0
    while x[index] == SPACE:
        count += 1
        if count > 10:
            return x
        index = rng.randint(0, length - 1)
    return x[:index] + x[index + 1:]


def add_letter(rng, x):                                                        # :103-114
    length = len(x)
    index = rng.randint(0, length - 1)
    count = 0
    while _is_space_or_digit(x[index]):
        count += 1
        if count > 10:
            return x
        index = rng.randint(0, length - 1)
    return x[:index] + [rng.choice(NEIGHBOURS[x[index]])] + x[index:]


def replace_letter(rng, x):                                                    # :117-128
    length = len(x)
    index = rng.randint(0, length - 1)
    count = 0
    while _is_space_or_digit(x[index]):
        count += 1
        if count > 10:
            return x
        index = rng.randint(0, length - 1)
    return x[:index] + [rng.choice(NEIGHBOURS[x[index]])] + x[index + 1:]


def _space_blocked(x, index):
    # x[index] == ' ', x[index - 1: index] in ('', ' '), x[index + 1: index + 2] in ('', ' ')   (:133)
    return x[index] == SPACE or x[index - 1] == SPACE or index + 1 >= len(x) or x[index + 1] == SPACE


def add_space(rng, x):                                                         # :131-143
    length = len(x)
    index = rng.randint(1, length - 1)
    count = 0
    while _space_blocked(x, index):
        count += 1
        if count > 10:
            return x
        index = rng.randint(1, length - 1)
    return x[:index] + [SPACE] + x[index:]


def remove_space(rng, x):                                                      # :146-154
    spaces = [i for i, c in enumerate(x) if c == SPACE]
    if not spaces:
        return x
    cut = rng.choice(spaces)
    return x[:cut] + x[cut + 1:]


def _words(x):
    words, word = [], []
    for c in x + [SPACE]:
        if c == SPACE:
            if word:
                words.append(word)
            word = []
        else:
            word.append(c)
    return words


def swap_word(rng, x):                                                         # :157-162
    words = _words(x)
    replace_index = rng.below(len(words))
    other_index = rng.below(len(words))
    words[replace_index], words[other_index] = words[other_index], words[replace_index]
    out = []
    for i, word in enumerate(words):
        out += ([SPACE] if i else []) + word
    return out


def transform_codes(x):
    """transform_title (common.py:20-47) on a title of codes: collapse runs of spaces, strip, cut to 255, strip,
    left-pad with '0' to 3 characters."""
    out = []
    for c in x:
        if c == SPACE and (not out or out[-1] == SPACE):
            continue
        out.append(c)
    while out and out[-1] == SPACE:
        out.pop()
    number_of_characters = len(out)
    out = out[:MAX_CHARACTERS]
    while out and out[-1] == SPACE:
        out.pop()
    if number_of_characters < N_GRAMS:
        out = [ZERO_DIGIT] * (N_GRAMS - len(out)) + out
    return out


def misspell_codes(codes, seed, index):
    """generate_misspelled_name (:165-173) of one title with the purpose-1 stream of `index`."""
    rng = Stream(seed, PURPOSE_MISSPELL, index)
    first = rng.choice([swap_word, add_letter, remove_letter])
    last = rng.choice([add_space, remove_space])
    functions = rng.sample([first, replace_letter, last], rng.randint(1, 2))
    word = list(codes)
    for function in functions:
        word = function(rng, word)
    return transform_codes(word)


def misspell(title, seed, index):
    return to_text(misspell_codes(to_codes(title), seed, index))


# ---- candidate sampling and row assembly (feature_engineering_prepare.py:25-57, feature_engineering.py:207-274) -------
def sample_candidates(candidates, sample_n, own, seed, index):
    """The sample of one train row (purpose-2 stream of its row number `index`): `sample_n` of the top-n candidates;
    for a row with a truth row of its own (own >= 0) that the sample misses, the last sampled candidate is replaced by
    it (:51-55).  Returns (truth rows, targets)."""
    sample = Stream(seed, PURPOSE_SAMPLE, index).sample(list(candidates), sample_n)
    if own >= 0 and own not in sample:
        sample = sample[:-1] + [own]
    return sample, [int(own >= 0 and row == own) for row in sample]


def row_plan(train_truth_rows):
    """The train rows that produce training rows, in output order: the rows with no truth row (-1), in row order
    (kind 2), then for each distinct truth row in order of first appearance the LAST train row holding it (kind 3)."""
    train_truth_rows = [int(r) for r in train_truth_rows]
    negative = [i for i, r in enumerate(train_truth_rows) if r < 0]
    last = {}
    for i, r in enumerate(train_truth_rows):
        if r >= 0:
            last[r] = i              # dict order: first appearance; value: the last row
    return negative, list(last.values())


def training_rows(truth_titles, train_truth_rows, top_rows, sample_n, seed):
    """(kind, query index, truth row, target, query title) per training row, in the reference's order.  truth_titles:
    transformed titles; train_truth_rows: the truth row of every train row's id (-1: not found); top_rows(i): the top-n
    truth rows of train row i in get_closest_matches order.  The query index is the train row (kinds 2, 3) or the truth
    row whose misspelling is the query (kind 1)."""
    negative, positive = row_plan(train_truth_rows)
    rows = []
    for kind, plan in ((KIND_NEGATIVE, negative), (KIND_POSITIVE, positive)):
        for i in plan:
            sample, target = sample_candidates(top_rows(i), sample_n, int(train_truth_rows[i]), seed, i)
            rows += [(kind, i, t, y, None) for t, y in zip(sample, target)]
    for t, title in enumerate(truth_titles):
        if len(title) > 9:                                    # feature_engineering.py:183-184
            rows.append((KIND_GENERATED, t, t, 1, misspell(title, seed, t)))
    return rows


def evaluation_split(kind, seed, generated=0.05, negative=0.10, positive=0.05):
    """_get_evaluation_indexes (feature_engineering.py:277-296) with a seeded NumPy generator: (train rows,
    evaluation rows), both ascending."""
    kind = np.asarray(kind)
    n = kind.shape[0]
    rng = np.random.default_rng(seed)
    chosen = []
    for name, code, fraction in (("generated", KIND_GENERATED, generated), ("negative", KIND_NEGATIVE, negative),
                                 ("positive", KIND_POSITIVE, positive)):
        candidates = np.nonzero(kind == code)[0]
        size = int(n * fraction)
        if size > candidates.shape[0]:
            raise ValueError(f"{name} rows: {candidates.shape[0]} < {size}")
        chosen.append(rng.choice(candidates, size, replace=False))
    evaluation = np.unique(np.concatenate(chosen)).astype(np.int64)
    train = np.setdiff1d(np.arange(n, dtype=np.int64), evaluation)
    return train, evaluation
