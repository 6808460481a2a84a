"""Java helpers needed host-side (key -> flowId for the Envoy RLS front end)."""


def string_hash_code(s: str) -> int:
    """java.lang.String.hashCode over UTF-16 code units (i32 wrap)."""
    h = 0
    data = s.encode("utf-16-le")
    for i in range(0, len(data), 2):
        cu = data[i] | (data[i + 1] << 8)
        h = (h * 31 + cu) & 0xFFFFFFFF
    return h - (1 << 32) if h >= (1 << 31) else h


def is_blank(s) -> bool:
    """StringUtil.isBlank: null, empty or only Character.isWhitespace chars (sentinel-core util/StringUtil.java:43-54)."""
    if not s:
        return True
    return all(c in " \t\n\x0b\f\r\x1c\x1d\x1e\x1f" or (c.isspace() and c not in "\x85\xa0\u2007\u202f")
               for c in s)


def double_to_string(x: float) -> str:
    """java.lang.Double.toString: the shortest digits that read back as x, always at least one fraction digit,
    computerized scientific notation ("1.0E7", "1.0E-4") at or above 1e7 and below 1e-3."""
    import math
    from decimal import Decimal
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    sign = "-" if math.copysign(1.0, x) < 0 else ""
    if x == 0:
        return sign + "0.0"
    _, digs, exp = Decimal(repr(abs(x))).as_tuple()
    digits = "".join(map(str, digs)).lstrip("0")
    exp += len(digits) - len(digits.rstrip("0"))
    digits = digits.rstrip("0")
    point = len(digits) + exp  # the value is 0.digits x 10^point
    if 1e-3 <= abs(x) < 1e7:
        if point <= 0:
            return sign + "0." + "0" * -point + digits
        whole = digits[:point].ljust(point, "0")
        return sign + whole + "." + (digits[point:] or "0")
    return sign + digits[0] + "." + (digits[1:] or "0") + "E" + str(point - 1)


def rls_key(domain: str, entries) -> str:
    """SentinelEnvoyRlsServiceImpl.generateKey: domain|k|v|k|v (RLS/SentinelEnvoyRlsServiceImpl.java:127-133)."""
    parts = [domain]
    for k, v in entries:
        parts.append(k)
        parts.append(v)
    return "|".join(parts)
