"""REGEX gateway items as byte-level DFAs for the parse kernel (k_gateway_parse's REGEX branch).

The oracle is `re.fullmatch(pattern, value)` on str -- what gateway.match_value and GatewayRuleManager.regex_bits
define as this project's REGEX behaviour.  compile_dfa turns a pattern of a regular subset into a DFA over UTF-8
bytes that accepts exactly the encodings of the strings fullmatch accepts; everything outside the subset, and
everything the parser is not sure of, gives None and the item stays on the host word.

  subset   literals (any code point), escaped punctuation, \\t \\n \\r \\f \\v \\xhh \\uhhhh \\Uhhhhhhhh, `.` (all but \\n),
           classes with ranges, negation and shorthands, \\d \\D \\w \\W \\s \\S, (...) (?:...) |, * + ? {m} {m,}
           {m,n} and their lazy forms (the same language under a full match)
  None     anchors, \\b \\B, backreferences, lookaround, possessive / atomic forms, inline flags, named groups,
           \\p{..} and every other escape, a `{` that does not open a counted repeat, nested-set lookalikes in a
           class, an NFA or DFA past its cap
  a pattern re.compile rejects -> the accept-all DFA (gateway._compile: no cache entry, the value is kept)

Every atom is a set of code point ranges without the surrogates (a value is UTF-8: it holds none); a set becomes
a byte automaton by the usual split of a range into 1- to 4-byte UTF-8 sequences, so `.` and negated classes
accept well-formed sequences only.  \\d \\w \\s are the sets `re` itself has in this interpreter, probed once per
process.  Thompson NFA over bytes -> subset construction -> minimisation -> bytes no state distinguishes merged
into classes.  State 0 is dead (not accepting, every transition to 0), state 1 the start.
"""
import re
import warnings
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_STATES = 4096          # design limits per pattern, not measurements: a u16 transition serves 65,535 states,
MAX_TABLE_BYTES = 1 << 20  # and a 1 MiB table still sits in the L2 beside the batch
MAX_CP = 0x10FFFF
_SUR_LO, _SUR_HI = 0xD800, 0xDFFF
Ranges = List[Tuple[int, int]]  # sorted, disjoint, inclusive code point ranges


@dataclass(eq=False)
class Dfa:
    n_states: int
    n_classes: int
    class_map: np.ndarray  # 256 x u8: byte -> class
    trans: np.ndarray      # n_states * n_classes x u16, row-major
    accept: np.ndarray     # (n_states + 7) // 8 x u8: bit (s & 7) of byte s >> 3

    def accepts(self, s: int) -> bool:
        return bool((int(self.accept[s >> 3]) >> (s & 7)) & 1)

    def match(self, b: bytes) -> bool:
        """The kernel's walk over the same tables."""
        s, nc, cm, tr = 1, self.n_classes, self.class_map.tolist(), self.trans.tolist()
        for x in b:
            s = tr[s * nc + cm[x]]
            if s == 0:
                return False
        return self.accepts(s)

    @property
    def table_bytes(self) -> int:
        return 256 + 2 * self.n_states * self.n_classes + len(self.accept)


# ---- code point sets
def _normalise(rs: Sequence[Tuple[int, int]]) -> Ranges:
    """Sorted, merged, surrogates removed."""
    out: Ranges = []
    for lo, hi in sorted(rs):
        if lo > hi:
            continue
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    cut: Ranges = []
    for lo, hi in out:
        if lo < _SUR_LO:
            cut.append((lo, min(hi, _SUR_LO - 1)))
        if hi > _SUR_HI:
            cut.append((max(lo, _SUR_HI + 1), hi))
    return [(lo, hi) for lo, hi in cut if lo <= hi]


def _negate(rs: Ranges) -> Ranges:
    out, at = [], 0
    for lo, hi in rs:
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= MAX_CP:
        out.append((at, MAX_CP))
    return _normalise(out)


_ALL = _normalise([(0, MAX_CP)])
_DOT = _normalise([(0, 9), (11, MAX_CP)])
_shorthand: Dict[str, Ranges] = {}


def shorthand_ranges(letter: str) -> Ranges:
    """The code points `re` matches with \\d, \\w or \\s (str patterns, no flags) in this interpreter, as ranges;
    the upper-case letters give the complements.  Probed once per process: every non-surrogate code point is put
    before the compiled shorthand."""
    if not _shorthand:
        text = "".join(map(chr, range(_SUR_LO))) + "".join(map(chr, range(_SUR_HI + 1, MAX_CP + 1)))
        for c in "dws":
            rs: Ranges = []
            for m in re.compile("\\" + c).finditer(text):
                i = m.start()
                cp = i if i < _SUR_LO else i + (_SUR_HI + 1 - _SUR_LO)
                if rs and rs[-1][1] == cp - 1:
                    rs[-1] = (rs[-1][0], cp)
                else:
                    rs.append((cp, cp))
            _shorthand[c] = _normalise(rs)
            _shorthand[c.upper()] = _negate(_shorthand[c])
    return _shorthand[letter]


# ---- UTF-8: a code point range as byte-range sequences
_UTF8_MAX = (0x7F, 0x7FF, 0xFFFF, MAX_CP)


def _utf8_sequences(lo: int, hi: int, out: list):
    """Appends the byte-range sequences ((lo, hi), ...) whose union is the UTF-8 encoding of [lo, hi] (no
    surrogates inside)."""
    for mx in _UTF8_MAX[:3]:
        if lo <= mx < hi:  # different lengths: split at the length boundary
            _utf8_sequences(lo, mx, out)
            _utf8_sequences(mx + 1, hi, out)
            return
    if hi <= 0x7F:
        out.append(((lo, hi),))
        return
    for i in (1, 2, 3):
        m = (1 << (6 * i)) - 1  # the low i continuation bytes
        if lo & ~m != hi & ~m:
            if lo & m:  # lo does not start a full block
                _utf8_sequences(lo, lo | m, out)
                _utf8_sequences((lo | m) + 1, hi, out)
                return
            if hi & m != m:  # hi does not end one
                _utf8_sequences(lo, (hi & ~m) - 1, out)
                _utf8_sequences(hi & ~m, hi, out)
                return
    a, b = chr(lo).encode("utf-8"), chr(hi).encode("utf-8")
    out.append(tuple(zip(a, b)))


# ---- the pattern: parsed into a small tree
# ("set", ranges) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)
class _Unsupported(Exception):
    """dialect: a construct of another dialect or a later re (a possessive or atomic form, which re compiles from
    Python 3.11 on; an escape letter such as \\p): a fallback whether or not this interpreter's re compiles it."""

    def __init__(self, dialect: bool = False):
        super().__init__()
        self.dialect = dialect


_META = set(".^$*+?{}[]\\|()")
_SIMPLE_ESC = {"t": 9, "n": 10, "r": 13, "f": 12, "v": 11}
_ASCII_ALNUM = set("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789")
_HEX = set("0123456789abcdefABCDEF")


class _Parser:
    def __init__(self, p: str):
        self.p, self.i = p, 0

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            raise _Unsupported  # an unbalanced ")"
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.repeat(self.atom()))
        return ("cat", items)

    def escape_cp(self, c: str) -> Optional[int]:
        """The code point of a single-character escape whose letter c was just consumed, None if c is none."""
        if c in _SIMPLE_ESC:
            return _SIMPLE_ESC[c]
        if c in "xuU":
            k = {"x": 2, "u": 4, "U": 8}[c]
            h = self.p[self.i:self.i + k]
            if len(h) != k or any(x not in _HEX for x in h) or int(h, 16) > MAX_CP:
                raise _Unsupported
            self.i += k
            return int(h, 16)
        if c not in _ASCII_ALNUM:
            return ord(c)  # re: a backslash before anything but an ASCII letter or digit is that character
        return None

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == ".":
            return ("set", _DOT)
        if c == "(":
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] != "?:":
                    # lookaround, flags, names, atomic groups, comments, conditionals
                    raise _Unsupported(dialect=self.p[self.i:self.i + 2] == "?>")
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                raise _Unsupported
            self.i += 1
            return node
        if c == "[":
            return ("set", self.klass())
        if c == "\\":
            e = self.peek()
            if not e:
                raise _Unsupported
            self.i += 1
            if e in "dDwWsS":
                return ("set", shorthand_ranges(e))
            cp = self.escape_cp(e)
            if cp is None:
                # \b \B \A \Z, backreferences, octal, \N{..}, \p{..}, ...; a letter re may not know either
                raise _Unsupported(dialect=not e.isdigit())
            return ("set", _normalise([(cp, cp)]))
        if c in "^$*+?{)|":
            raise _Unsupported  # anchors; a repeat of nothing; a `{` that is not a repeat
        return ("set", _normalise([(ord(c), ord(c))]))  # "}" and "]" alone are literals in re

    def klass(self) -> Ranges:
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        rs, first = [], True
        while True:
            c = self.peek()
            if not c:
                raise _Unsupported
            self.i += 1
            if c == "]" and not first:
                break
            first = False
            if c == "[" or (c in "-&~|" and self.peek() == c):
                raise _Unsupported  # re warns of a possible nested set / set operation: not guessed at
            lo = self.class_member(c, rs)
            if lo is None:  # a shorthand
                if self.peek() == "-" and self.p[self.i + 1:self.i + 2] != "]":
                    raise _Unsupported
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                d = self.peek()
                self.i += 1
                if d == "[":
                    raise _Unsupported
                hi = self.class_member(d, None)
                if hi is None or hi < lo:
                    raise _Unsupported
                rs.append((lo, hi))
            else:
                rs.append((lo, lo))
        rs = _normalise(rs)
        return _negate(rs) if neg else rs

    def class_member(self, c: str, rs) -> Optional[int]:
        """One member of a class whose first character c was consumed: its code point, or None after adding a
        shorthand's ranges to rs (rs None: a shorthand is not allowed here)."""
        if c != "\\":
            return ord(c)
        e = self.peek()
        if not e:
            raise _Unsupported
        self.i += 1
        if e in "dDwWsS":
            if rs is None:
                raise _Unsupported
            rs.extend(shorthand_ranges(e))
            return None
        cp = self.escape_cp(e)
        if cp is None:
            raise _Unsupported  # \b is a backspace here, octal, ...: not taken
        return cp

    def repeat(self, node):
        c = self.peek()
        if c in ("*", "+", "?"):
            self.i += 1
            m, n = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
        elif c == "{":
            j = self.p.find("}", self.i)
            body = self.p[self.i + 1:j] if j > 0 else ""
            mo = re.fullmatch(r"([0-9]+)(,([0-9]*))?", body, re.ASCII)
            if not mo:
                raise _Unsupported  # a literal "{" (or {,n}): left to the host
            self.i = j + 1
            m = int(mo.group(1))
            n = m if mo.group(2) is None else (int(mo.group(3)) if mo.group(3) else None)
            if n is not None and n < m:
                raise _Unsupported
        else:
            return node
        if self.peek() == "?":
            self.i += 1  # lazy: the same language
        if self.peek() in ("*", "+", "?", "{"):
            raise _Unsupported(dialect=self.peek() == "+")  # possessive, or a repeat of a repeat
        return ("rep", node, m, n)


# ---- Thompson NFA over bytes
class _TooBig(Exception):
    pass


class _Nfa:
    def __init__(self, cap: int):
        self.cap = cap
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int, int]]] = []  # (lo, hi, target)

    def state(self) -> int:
        if len(self.eps) >= self.cap:
            raise _TooBig
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node, start: int) -> int:
        """Adds node's automaton leaving `start`; returns its end state."""
        kind = node[0]
        if kind == "set":
            end = self.state()
            seqs: list = []
            for lo, hi in node[1]:
                _utf8_sequences(lo, hi, seqs)
            trie: Dict[Tuple[int, int, int], int] = {}  # shared prefixes: (state, lo, hi) -> state
            for seq in seqs:
                at = start
                for k, (lo, hi) in enumerate(seq):
                    if k == len(seq) - 1:
                        self.edges[at].append((lo, hi, end))
                    else:
                        nxt = trie.get((at, lo, hi))
                        if nxt is None:
                            nxt = trie[(at, lo, hi)] = self.state()
                            self.edges[at].append((lo, hi, nxt))
                        at = nxt
            return end
        if kind == "cat":
            for sub in node[1]:
                start = self.build(sub, start)
            return start
        if kind == "alt":
            end = self.state()
            for sub in node[1]:
                s = self.state()
                self.eps[start].append(s)
                self.eps[self.build(sub, s)].append(end)
            return end
        _, sub, m, n = node
        for _ in range(m):
            start = self.build(sub, start)
        if n is None:  # sub*
            loop = self.state()
            self.eps[start].append(loop)
            body = self.state()
            self.eps[loop].append(body)
            self.eps[self.build(sub, body)].append(loop)
            return loop
        end = self.state()
        self.eps[start].append(end)
        for _ in range(n - m):  # (sub (sub (...)?)?)?
            s = self.state()
            self.eps[start].append(s)
            start = self.build(sub, s)
            self.eps[start].append(end)
        return end


def _determinise(nfa: _Nfa, start: int, final: int, max_states: int):
    """Subset construction over the byte classes of the NFA's edges: (class of each byte, rows, accepting), state 0
    the empty set."""
    cuts = {0}
    for es in nfa.edges:
        for lo, hi, _ in es:
            cuts.add(lo)
            cuts.add(hi + 1)
    cuts.discard(256)
    bounds = sorted(cuts)
    byte_class = np.zeros(256, dtype=np.int64)
    for k, b in enumerate(bounds):
        byte_class[b:] = k
    nc = len(bounds)
    cls_of = byte_class.tolist()

    closure_of: Dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out = set()
        for s in states:
            c = closure_of.get(s)
            if c is None:
                seen, stack = {s}, [s]
                while stack:
                    for t in nfa.eps[stack.pop()]:
                        if t not in seen:
                            seen.add(t)
                            stack.append(t)
                c = closure_of[s] = frozenset(seen)
            out |= c
        return frozenset(out)

    ids = {frozenset(): 0}
    first = closure([start])
    ids[first] = 1
    order = [frozenset(), first]
    rows = [[0] * nc]
    at = 1
    while at < len(order):
        targets: List[Optional[set]] = [None] * nc
        for s in order[at]:
            for lo, hi, t in nfa.edges[s]:
                for k in range(cls_of[lo], cls_of[hi] + 1):
                    if targets[k] is None:
                        targets[k] = {t}
                    else:
                        targets[k].add(t)
        row = [0] * nc
        memo: Dict[frozenset, int] = {}
        for k, tg in enumerate(targets):
            if tg is None:
                continue
            key = frozenset(tg)
            d = memo.get(key)
            if d is None:
                cl = closure(key)
                d = ids.get(cl)
                if d is None:
                    if len(order) >= max_states:
                        raise _TooBig
                    d = ids[cl] = len(order)
                    order.append(cl)
                memo[key] = d
            row[k] = d
        rows.append(row)
        at += 1
    accepting = [final in st for st in order]
    return byte_class, np.array(rows, dtype=np.int64).reshape(len(order), nc), np.array(accepting, dtype=bool)


def _minimise(rows: np.ndarray, accepting: np.ndarray):
    """Moore's refinement: (block of each state, number of blocks).  States that reach no accepting state end in
    the dead state's block."""
    block = accepting.astype(np.int64)
    n_blocks = len(np.unique(block))
    while True:
        sig = np.concatenate([block[:, None], block[rows]], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = new.reshape(-1)
        k = int(new.max()) + 1
        if k == n_blocks:
            return new, k
        block, n_blocks = new, k


def _accept_all() -> Dfa:
    return Dfa(2, 1, np.zeros(256, np.uint8), np.array([0, 1], np.uint16), np.array([2], np.uint8))


def compile_dfa(pattern: str, max_states: int = MAX_STATES, max_table_bytes: int = MAX_TABLE_BYTES) -> Optional[Dfa]:
    """The DFA of `pattern` over UTF-8 bytes, None when the pattern is outside the subset or its automaton passes a
    cap (max_states bounds the subset construction and so the result; the NFA may hold 32 states per allowed DFA
    state), the accept-all DFA when re.compile rejects the pattern."""
    tree = dialect = None
    try:
        tree = _Parser(pattern).parse()
    except _Unsupported as u:
        dialect = u.dialect
    except RecursionError:
        pass
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            re.compile(pattern)
    except re.error:
        return None if dialect else _accept_all()
    except Exception:
        return None
    if tree is None:
        return None
    try:
        nfa = _Nfa(32 * max(1, max_states))
        start = nfa.state()
        final = nfa.build(tree, start)
        byte_class, rows, accepting = _determinise(nfa, start, final, max_states)
    except (_Unsupported, _TooBig, RecursionError):
        return None
    block, n_blocks = _minimise(rows, accepting)
    # renumber: the dead block 0, the start block 1 (a start that is dead gets a dead row of its own)
    dead, first = int(block[0]), int(block[1])
    number = {dead: 0}
    if first != dead:
        number[first] = 1
    n_states = 2
    for b in block.tolist():
        if b not in number:
            number[b] = n_states
            n_states += 1
    table = np.zeros((n_states, rows.shape[1]), dtype=np.int64)
    acc = np.zeros(n_states, dtype=bool)
    for s in range(len(block)):
        d = number[int(block[s])]
        if d == 0:
            continue
        table[d] = [number[int(block[t])] for t in rows[s]]
        acc[d] = accepting[s]
    # bytes with equal columns share a class
    cols, col_class = np.unique(table, axis=1, return_inverse=True)
    col_class = col_class.reshape(-1)
    n_classes = cols.shape[1]
    if n_states > min(max_states, 65535) or 256 + 2 * n_states * n_classes + (n_states + 7) // 8 > max_table_bytes:
        return None
    accept = np.packbits(acc, bitorder="little")
    return Dfa(n_states, n_classes, col_class[byte_class].astype(np.uint8),
               np.ascontiguousarray(cols, dtype=np.uint16).reshape(-1), accept.astype(np.uint8))
