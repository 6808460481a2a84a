"""TEST INFRASTRUCTURE: the pattern and value corpus of the device-REGEX tests (tests/test_gateway_regex_host.py,
tests/test_gateway_regex_gpu.py).  The expected side is always re.fullmatch."""
import random

CLEF = "\U0001D11E"   # 4 bytes
DIGIT3 = "٣"     # ARABIC-INDIC DIGIT THREE: \d and \w, 2 bytes
EMSPACE = " "    # \s, 3 bytes
# 1-, 2-, 3- and 4-byte characters, the patterns' own letters, the shorthands' Unicode members and "\n"
ALPHABET = ["a", "b", "1", "é", "€", CLEF, DIGIT3, EMSPACE, "\n", "-"]

PATTERNS = [
    # literals and escapes
    r"a", r"ab", r"é", "€" + CLEF, r"a\-b", r"\x61é", r"\U0001D11Ea?", r"\n", r"\t|\r|\f|\v|\n", r"\é", r"a\|b",
    r"]", r"a}", r"€+",
    # the dot
    r".", r".*", r".+", r"a.b", r"..", r"(?:.|\n)*", r".?.?.?",
    # classes
    r"[ab]", r"[ab]*", r"[^a]", r"[^a]*", r"[^ab1]+", "[é€" + CLEF + "]", "[é€" + CLEF + "]+", "[^é€" + CLEF + "]*",
    r"[a-b1-1]+", r"[\d\s]*", r"[^\d\s]*", r"[\w-]+", r"[]a]*", r"[^]a]*", r"[a\-b]*", r"[-a]*", r"[a-]*",
    r"[\x61-\x62]+", "[٠-٩]+", r"[^\n]*", r"[\W]*", r"[\D]+", r"[\S\n]*",
    # shorthands
    r"\d", r"\d+", r"\D*", r"\w", r"\w*", r"\W+", r"\s", r"\s*", r"\S*", r"\w+\s\w+", r"\d*\D\d*",
    # groups and alternation, unequal lengths
    r"(a|ab)(b|)", r"(?:a|b|é€)*", r"(a|b)*a", r"a|ab|abb|", r"(|a)(|b)(|1)", r"((a|b)|(é|€))+", r"(?:(?:a)|(?:\w\w))*",
    r"(.|\s)(.|\s)?", r"(a|[^a])*",
    # repeats, counted and lazy
    r"x*", r"a?", r"a+", r"a*b*", r"a{0}", r"a{0}b", r"a{0,1}", r"a{2,}", r"a{2,4}", r"[ab]{2}", r"(?:ab){1,2}",
    r".{0,3}", r".{2,}", r"\w{1,3}", r"a*?", r"a+?b", r"a??b", r"[ab]{1,2}?", r".*?a", r"(?:a*)*", r"(?:a|b*)+",
    r"(a?){3}", r"\S{0,2}\s?",
]

# the constructs that stay on the host word
FALLBACKS = [r"^a", r"a$", r"\bfoo", r"a\B", r"(a)\1", r"(?=a)a", r"(?!a)b", r"(?<=a)b", r"(?i)a", r"(?s:.)",
             r"(?P<n>a)", r"\Aa", r"a\Z", r"\141", r"[\b]", r"[[a]", r"\N{BULLET}", r"(?#c)a", r"a{,2}"]
# what re compiles from Python 3.11 on only, or not at all: a fallback on every version
DIALECT = [r"a*+", r"a++", r"a?+", r"a{2}+", r"(?>a)", r"\p{L}", r"\P{Lu}a"]
UNCOMPILABLE = [r"a**", r"(", r")", r"[a", r"a{2}{3}", r"*a", r"[b-a]"]

VALUES = ["", "a", "b", "ab", "abb", "aa", "aaa", "aaaa", "aaaaa", "ba", "1", "12", "é", "€", CLEF, "é€", "€" + CLEF,
          "\n", "a\n", "\na", "a\nb", "axb", "a-b", DIGIT3, "1" + DIGIT3, " ", "a b", EMSPACE, "a" + EMSPACE + "b", "\t",
          "]", "]a", "a}", "a|b", "-", "a-", "x", "xx", "éa", "aé", "1a1", "a1", "_", CLEF + "a", "\r", "\x0b", "\x1c",
          "\x85", "\xa0", "€€", "ab" * 20, ("é€" + CLEF + "a") * 8, "a" * 255]


def random_values(n=600, seed=7):
    """Short strings over ALPHABET, every other one over its three ASCII letters only, so that accepts are common."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        alpha = ALPHABET[:3] if i % 2 else ALPHABET
        out.append("".join(rng.choice(alpha) for _ in range(rng.randrange(0, 5))))
    return out
