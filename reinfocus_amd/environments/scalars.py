"""Scalar parameters of the strategy classes, kept to the numpy 1.26 promotion the reference pins (numpy ~= 1.26.4).

The strategy classes mix float32 (or bool) arrays with scalar parameters.  Under numpy 1.26's value-based casting a
Python float and a numpy.float64 behave alike: next to a float32 array both are cast to float32, next to a bool array
both give float64.  Under NEP 50 (numpy 2) a numpy.float64 is "strong" and turns float32 arithmetic into float64, so
`parameter` makes it a Python float, which is weak under NEP 50 and behaves as numpy 1.26's numpy.float64 did.  A
numpy.float32 stays one: next to arrays both numpy versions treat it alike (a bool array times it is float32).  Numpy
integers become Python ints for the same reason.

Where two parameters meet each other (on - off, high - low, the two limits), numpy 1.26 computes in float32 only when
both are numpy.float32 and in float64 otherwise; NEP 50 would keep a numpy.float32 next to a Python float in float32.
`difference` computes as numpy 1.26 does.

Value-based casting keeps a float parameter in float32 only while its magnitude is below 3.4e38; NEP 50 always does.
Finite parameters at or past that bound are refused (AssertionError), and so are numpy floating types other than
float32 and float64.  Infinities and NaN pass here; the device program compiler refuses them.
"""

import math

import numpy as np

FLOAT32_BOUND = 3.4e38  # numpy 1.26 value-based casting: |x| < this fits float32 (min_scalar_type)


def _in_range(x, what):
    if isinstance(x, float) and math.isfinite(x):
        assert abs(x) < FLOAT32_BOUND, f"{what}: {x!r} is outside the float32 range numpy 1.26 casts to float32"
    return x


def parameter(x, what="parameter"):
    """A scalar parameter as numpy 1.26 would use it, under any numpy (see the module docstring)."""
    if isinstance(x, np.floating):
        assert isinstance(x, (np.float32, np.float64)), f"{what}: {type(x).__name__} scalars are not supported"
        if isinstance(x, np.float64):
            x = float(x)
    elif isinstance(x, np.integer):
        x = int(x)
    return _in_range(x, what)


def difference(a, b, what="parameter"):
    """a - b of two normalised parameters with numpy 1.26's scalar promotion."""
    if isinstance(a, np.float32) and isinstance(b, np.float32):
        return a - b
    if isinstance(a, np.float32) or isinstance(b, np.float32):
        return _in_range(float(a) - float(b), what)
    return _in_range(a - b, what)
