"""The argument rule of the strict mesh stages, once: an integer is an `int` or `np.integer` and no bool, a number is
real, finite and no bool, each within what the stage allows; anything else is a ValueError that names the parameter and shows the value.
The `_checked_*` functions of the stages are calls of these two.
"""
import math

import numpy as np


def integer(name, value, lo, hi, span=None):
    """value as an int, or a ValueError: no bool, an int or np.integer, in lo..hi.  span words the range where a stage has its own text for
    it ('1..2^31 - 1')."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError('{} must be an integer in {}, got {!r}'.format(name, span or '{}..{}'.format(lo, hi), value))
    return int(value)


def number(name, value, ok, rule):
    """value as a float, or a ValueError: no bool, an int, float, np.integer or np.floating, finite, and ok(float) holds.  rule words all of
    that ('a finite number > 0')."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(value) \
            or not ok(float(value)):
        raise ValueError('{} must be {}, got {!r}'.format(name, rule, value))
    return float(value)
