"""Definitions and lines for the hop tier's tests (tests/test_hop_host.py, tests/test_gpu_hop.py) and tools/fuzz_hop.py: not a
conftest, nothing here runs a kernel.

gorp_amd.workloads.syslog_definition is one family: one literal trie, \\d+ / \\w+ / \\S+ values, blanks between them.
fielded_definition draws definitions of the same kind of text -- an opening literal, then fields and separators -- from fourteen
field patterns and eighteen separators, so that runs over other intervals, loop sets of other shapes, chains with a NUL or a
byte above 0x7F in them and tail sets of other fields come out, and makes the lines that go with them.

Lines are str of code points below 0x100 (one byte each as latin-1) unless a test widens them itself."""
import string

LOWER, UPPER, DIGITS = string.ascii_lowercase, string.ascii_uppercase, string.digits
PRINTABLE = "".join(chr(c) for c in range(0x21, 0x7F))      # (no blank)
HIGH = "\xe9\xff\x80\xb7"

# A definition's text goes to the library (and to the oracle) as a C string, so a literal cannot hold a NUL.  A class that holds
# nothing else can: every unit but U+0000 taken out.
NUL_CLASS = "[^\x01-\uffff]"


class Field:
    """One field pattern: rx; `lower`, the alphabet of its heaviest interval (what a state's run covers); `mixed`, an alphabet over every
    interval of its class; whether the class admits a byte above 0x7F; `inside`, the class of its last repeated element as a predicate
    on a character (what a separator behind it must not begin with); length limits of a value."""

    def __init__(self, rx, lower, mixed, high, inside, lo=1, hi=40, make=None):
        self.rx, self.lower, self.mixed, self.high, self.inside, self.lo, self.hi, self.make = rx, lower, mixed, high, inside, lo, hi, make

    def value(self, rng, style, stretch=0):
        if self.make is not None:
            return self.make(rng, style)
        hi = max(stretch, self.hi) if self.hi == 40 else self.hi       # (stretch: long lines for the slice kernel)
        n = rng.randint(self.lo, hi) if rng.random() < 0.5 else rng.randint(self.lo, min(hi, 8))
        alphabet = self.lower if style == "lower" else self.mixed
        v = [rng.choice(alphabet) for _ in range(n)]
        if style != "lower" and rng.random() < 0.4:
            # a value that begins with a digit or an upper-case letter: the chain into it ends in the tail SET, not the tail interval
            first = [ch for ch in DIGITS + UPPER if ch in self.mixed]
            if first:
                v[0] = rng.choice(first)
        if style == "high" and self.high:
            v[rng.randrange(n)] = rng.choice(HIGH)
        return "".join(v)


def _not_in(chars):
    return lambda ch: ch not in chars


def _decimal(rng, style):
    return "".join(rng.choice(DIGITS) for _ in range(rng.randint(1, 20))) + "." + "".join(rng.choice(DIGITS) for _ in range(rng.randint(1, 19)))


_WORD = LOWER + UPPER + DIGITS + "_"
_SPACES = " \t\n\r\f\x0b\x08"
FIELDS = [
    Field("\\d+", DIGITS, DIGITS, False, lambda ch: ch in DIGITS),
    Field("\\w+", LOWER, _WORD, False, lambda ch: ch in _WORD),
    Field("\\S+", LOWER, PRINTABLE, True, _not_in(_SPACES)),
    Field("[^,]+", LOWER, (PRINTABLE + " ").replace(",", ""), True, _not_in(",")),
    Field("[^\\s\"]+", LOWER, PRINTABLE.replace("\"", ""), True, _not_in(_SPACES + "\"")),
    Field("[a-f0-9]+", "abcdef", "abcdef" + DIGITS, False, lambda ch: ch in "abcdef" + DIGITS),
    Field("[A-Z]+", UPPER, UPPER, False, lambda ch: ch in UPPER),
    Field("\\d+\\.\\d+", DIGITS, DIGITS, False, lambda ch: ch in DIGITS, make=_decimal),
    Field("(GET|PUT|POST)", "", "", False, lambda ch: False, make=lambda rng, style: rng.choice(["GET", "PUT", "POST"])),
    Field("[\\w.-]+", LOWER, _WORD + ".-", False, lambda ch: ch in _WORD + ".-"),
    Field("\\d{1,3}", DIGITS, DIGITS, False, lambda ch: ch in DIGITS, hi=3),
    Field("[a-z]{2,}", LOWER, LOWER, False, lambda ch: ch in LOWER, lo=2),
    Field("[^\\]]+", LOWER, (PRINTABLE + " ").replace("]", ""), True, _not_in("]")),
    Field(".+?", LOWER, PRINTABLE + " ", True, lambda ch: True),
]


def T(s):
    return ["text", s]


# (pieces of the definition, the text a well-formed line has there).  A blank in a template is [ \t]+.
SEPARATORS = [([T(s)], s) for s in (" ", "  ", ", ", ",", " = ", "=", ": ", "; k=", " [", "] ", "\t", " - ", "\" \"", "|", " user=", " took ")] + [
    ([["pattern", NUL_CLASS], T(";")], "\x00;"),          # a NUL byte, then ';'
    ([T(" \xb7 ")], " \xb7 "),                             # a byte above 0x7F between two blanks
]


def _begins(sep_text):
    """The characters a separator may begin with in a line (a blank: a tab as well)."""
    return " \t" if sep_text[0] in " \t" else sep_text[0]


def admissible(field, sep):
    """The rule that keeps a capture's end decidable in one pass (what the hop tier needs: it refuses general capture programs, gx_stat 26
    == 2): no character a separator can begin with lies in the class of the field before it."""
    return not any(field.inside(ch) for ch in _begins(sep[1]))


def _opening(rng, taken):
    while True:
        word = "".join(rng.choice(LOWER + UPPER + DIGITS + "_-.") for _ in range(rng.randint(2, 9)))
        if word not in taken:
            taken.add(word)
            return rng.choice(["", "", "<", "[", "svc "]) + word + rng.choice([" ", ": ", "=", "[", " - "])


def fielded_definition(rng, n_extractions):
    """(rules, makers): n_extractions extractions, each an opening literal of its own and 1-5 fields with separators between them, half
    of them ending on a field and half on a separator; makers[k](rng, style="lower" | "mixed" | "high", stretch=0) is a well-formed
    line of extraction k: values of 1-40 characters (up to `stretch` where that is more and the pattern sets no limit), "lower" inside the
    heaviest interval of the field's class, "mixed" over all of them, "high" with a byte above 0x7F in the values whose class admits one."""
    from gorp_amd.gorp import FlattenedExtraction
    rules, makers, taken = [], [], set()
    for k in range(n_extractions):
        opening = _opening(rng, taken)
        pieces, parts = [T(opening)], [opening]      # parts: str (text as it is) or Field (a value)
        n_fields, ends_on_field = rng.randint(1, 5), k % 2 == 0
        for j in range(n_fields):
            f = rng.choice(FIELDS)
            rx = ["pattern", f.rx]
            pieces.append(rx if rng.random() < 0.2 else ["extractor", "f%d" % j, [rx]])
            parts.append(f)
            seps = [s for s in SEPARATORS if admissible(f, s)]
            last = j + 1 == n_fields or not seps
            if seps and not (last and ends_on_field):
                sep = rng.choice(seps)
                pieces += sep[0]
                parts.append(sep[1])
            if last:
                break
        rules.append(FlattenedExtraction("x%d" % k, pieces))
        makers.append(lambda rng, style="lower", stretch=0, parts=parts: "".join(p if isinstance(p, str) else p.value(rng, style, stretch) for p in parts))
    return rules, makers


def fielded(n_extractions, seed):
    """The fielded definition the tests use at a size and seed: (rules, makers, the generator as the draw left it)."""
    import random
    rng = random.Random(1000 * n_extractions + seed)
    rules, makers = fielded_definition(rng, n_extractions)
    return rules, makers, rng


_REPLACEMENTS = "_Z9\x7f\xe9=[]: \x00"


def damage(rng, line):
    """One of the kinds of damage the hop walk has a branch for: blanks doubled or tabbed ([ \\t]+: a chain assumes one blank), the line
    cut short (inside a run, a chain, the trie), one byte replaced (NUL and 0x7F among the replacements), a stretch repeated."""
    r = rng.random() * 0.7
    if r < 0.2:
        return line.replace(" ", rng.choice(["  ", "\t", " \t "]), rng.randint(1, 4))
    if r < 0.4:
        return line[:rng.randint(0, len(line))]
    if not line:
        return line
    k = rng.randrange(len(line))
    if r < 0.6:
        return line[:k] + rng.choice(_REPLACEMENTS) + line[k + 1:]
    return line[:k] + line[k:k + rng.randint(1, 30)] * rng.randint(2, 9) + line[k:]


def cut_pairs(line):
    """For every c in 0..len(line): line[:c], then line[c:] -- to be laid next to each other in a batch, in this order, so that behind the
    cut line's end lie exactly the bytes the automaton would take next."""
    for c in range(len(line) + 1):
        yield line[:c]
        yield line[c:]


def utf16_csr(lines):
    """A list of str as a UTF-16 batch: (units uint16[total], offsets uint32[n + 1])."""
    import numpy as np
    units = [np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16) for s in lines]
    offsets = np.zeros(len(lines) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(u) for u in units])
    return np.concatenate([u for u in units if len(u)] or [np.zeros(0, np.uint16)]), offsets


def oracle_rows(orc, lines, max_groups):
    """The oracle's answers for a list of str, line by line on the Strings (what a UTF-16 batch is compared with): (ids, offsets)."""
    import numpy as np
    ids = np.empty(len(lines), np.int32)
    caps = np.full((len(lines), 2 * max_groups), -1, np.int32)
    for i, s in enumerate(lines):
        mid, spans = orc.extract(s)
        ids[i] = mid
        for g, span in enumerate(spans):
            if span is not None:
                caps[i, 2 * g], caps[i, 2 * g + 1] = span
    return ids, caps
