"""A banded unit-cost edit distance in plain numpy: the reference for arms too long for the oracle's full matrix.

Only the diagonals -band .. +band of each row are kept, so an arm pair of 60 000 bases costs 60 000 short vector steps
instead of 3.6 * 10^9 cells.  The value is exact whenever it is at most `band`: an alignment of cost d <= band never
leaves the diagonals -d .. +d, so the best path inside the band is the best path; and a banded value <= band is the cost
of a real alignment, hence an upper bound of the true distance, which then lies within the band as well.  Anything
larger is reported as None, never as a number.

tests/test_gpu_score_reach.py validates this against the oracle's full matrix before it relies on it."""
import numpy as np

_FAR = 1 << 40                                  # "no cell here"; far above any distance, far below an int64 overflow
_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _x, _y in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMPLEMENT[_x] = _y


def oriented(b, flag):
    """The right arm as ComputeScore walks it (src/structs.rs:443-448): reversed (bit 0), then complemented (bit 1)."""
    b = np.asarray(b, dtype=np.uint8)
    if flag & 1:
        b = b[::-1]
    if flag & 2:
        b = _COMPLEMENT[b]
    return b


def as_flag(b, flag):
    """The bytes to write into the text so that the right arm, walked with `flag`, reads b (both steps are involutions
    and commute)."""
    return np.ascontiguousarray(oriented(b, flag))


def identity_f32(distance, left_length, right_length):
    """ProtoSD::levenshtein's value from a distance: f64 arithmetic over the longer LENGTH, then `as f32`."""
    return np.float32(100.0 * (1.0 - distance / max(left_length, right_length)))


def banded_distance(a, b, band):
    """Unit-cost edit distance of the byte arrays a and b when it is at most `band`, else None.

    Row i holds D[i][i + d] for d = -band .. band at index d + band.  From row i - 1: the diagonal neighbour has the same
    index, the upper one index + 1; the left neighbour is in the row itself and is folded in as a running minimum,
    cur[k] = min over k' <= k of (cand[k'] + k - k')."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    la, lb, w = len(a), len(b), 2 * band + 1
    if abs(la - lb) > band:
        return None
    s = np.arange(w, dtype=np.int64)
    d = s - band
    # bp[i + k] = b[i + d[k] - 1], the base of column j = i + d[k]; columns outside 1 .. lb read padding and are masked
    # (the last row is at most lb + band: its window ends 2 band + 1 entries behind b)
    bp = np.concatenate([np.zeros(band + 1, np.uint8), b, np.zeros(2 * band + 1, np.uint8)])
    prev = np.where(d >= 0, d, _FAR)            # row 0: D[0][j] = j
    prev[d > lb] = _FAR
    up = np.empty(w, dtype=np.int64)
    up[-1] = _FAR                               # the cell above the band's last diagonal is outside the band
    for i in range(1, la + 1):
        cand = prev + (bp[i:i + w] != a[i - 1])
        up[:-1] = prev[1:]
        np.minimum(cand, up + 1, out=cand)
        if i <= band or i + band > lb:          # the band sticks out of the matrix: column 0 is i, the rest is no cell
            j = d + i
            cand[(j < 1) | (j > lb)] = _FAR
            cand[j == 0] = i
        cand -= s
        np.minimum.accumulate(cand, out=cand)
        cand += s
        prev = cand
    dist = int(prev[lb - la + band])
    return dist if dist <= band else None
