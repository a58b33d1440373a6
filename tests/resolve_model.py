"""The supersampled resolve, in NumPy, written from the text of include/swr.h ("Supersampled resolve") alone.  A plain helper module of
tests/test_resolve.py (not a conftest, not a test file).  Its inputs are images a test wrote itself or frames of the CPU oracle; it is
never fed by the library.

    colour   out = (sum of the S*S bytes of the block + S*S/2) / (S*S), integer division, per channel
    depth    SAMPLE0: the bits of sample (0,0);  MIN: m = sample (0,0), then the others in row-major order,
             if (s < m || (m != m && s == s)) m = s — the bits of m
"""
import numpy as np

SAMPLE0, MIN = 0, 1


def color(src, S):
    """(H, W, 4) uint8 -> (H/S, W/S, 4) uint8."""
    src = np.asarray(src)
    H, W = src.shape[:2]
    assert src.dtype == np.uint8 and H % S == 0 and W % S == 0
    total = np.zeros((H // S, W // S, 4), dtype=np.int64)
    for j in range(S):
        for i in range(S):
            total += src[j::S, i::S]
    return ((total + S * S // 2) // (S * S)).astype(np.uint8)


def depth(src, S, depth_filter):
    """(H, W) float32 -> (H/S, W/S) float32, bits kept (compare with .tobytes() or a uint32 view)."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    H, W = src.shape
    assert H % S == 0 and W % S == 0
    bits = src.view(np.uint32)
    mb = bits[0::S, 0::S].copy()
    if depth_filter == SAMPLE0:
        return mb.view(np.float32)
    assert depth_filter == MIN
    for j in range(S):
        for i in range(S):
            if i == 0 and j == 0:
                continue
            m = mb.view(np.float32)
            s, sb = src[j::S, i::S], bits[j::S, i::S]
            with np.errstate(invalid="ignore"):
                take = (s < m) | ((m != m) & (s == s))
            mb = np.where(take, sb, mb)
    return np.ascontiguousarray(mb).view(np.float32)


def partial_fraction(resolved_color):
    """The share of pixels whose alpha (the coverage) is strictly between 0 and 255."""
    a = np.asarray(resolved_color)[..., 3]
    return float(((a > 0) & (a < 255)).mean())
