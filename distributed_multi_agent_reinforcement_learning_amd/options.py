"""The validators the option parsers share.  `section` is cfg.algo or cfg.runtime, `key` the full name ("algo.bc_beta") that the
ValueError carries; the entry read is the part of `key` behind the first dot."""
import math


def real(section, key, default):
    raw = section.get(key.partition(".")[2], default)
    if isinstance(raw, bool) or not isinstance(raw, (int, float)) or not math.isfinite(raw):
        raise ValueError(f"{key}: {raw!r} is not a finite number")
    return float(raw)


def flag(section, key, default):
    raw = section.get(key.partition(".")[2], default)
    if not isinstance(raw, bool):
        raise ValueError(f"{key}: {raw!r} is not true or false")
    return raw


def count(section, key, default=0):
    raw = section.get(key.partition(".")[2], default)
    if isinstance(raw, bool) or not isinstance(raw, int) or raw < 0:
        raise ValueError(f"{key}: {raw!r} is not an integer >= 0")
    return raw


def distance(section, key, default=None):
    """a length of the scripted pursuers' settings: anything float() takes, finite and >= 0; None (absent) stays None"""
    raw = section.get(key.partition(".")[2], default)
    if raw is None:
        return None
    try:
        v = float(raw)
    except (TypeError, ValueError):
        raise ValueError(f"{key}: {raw!r} is not a number") from None
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{key}: {v} is not a finite number >= 0")
    return v
