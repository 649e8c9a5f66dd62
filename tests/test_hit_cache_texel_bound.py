"""Why no frame of the sphere world raises SFRT_E_TEXEL's bit, from a marching launch or from one
that reads the hit cache (tests/test_hit_cache.py): sphere_trace.hip shade_texel takes a column
as trunc(f * tw) and a row as trunc(g * th) in binary32, f and g fractions v - trunc(v) of
non-negative v (or NaN, which converts to 0), so f, g <= 1 - 2^-24; the index column + row * tw
leaves the texture only if such a product rounds up to the size itself.  For every size a
texture can have (1 .. 65535, 16 bits of SphereRec::tex_wh) it does not: the product lies more
than half an ulp below the size unless the size is a power of two, where it is representable."""
import numpy as np


def test_largest_fraction_times_size_stays_below_size():
    size = np.arange(1, 65536, dtype=np.float32)
    f = np.nextafter(np.float32(1), np.float32(0))  # the largest binary32 below 1
    assert f == np.float32(1) - np.float32(2.0 ** -24)
    prod = f * size  # binary32, round to nearest even, as v_mul_f32
    assert prod.dtype == np.float32
    assert (prod < size).all()
    assert (np.trunc(prod) <= size - 1).all()  # monotone in f: every smaller fraction too
