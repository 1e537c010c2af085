"""An independent restatement of the library's counter-based dropout stream (csrc/common.h:
mms_mix32, mms_hash, mms_keep, mms_drop_thresh), written from the text of the header with integer
operations only (numpy uint64 with 32-bit masking).  It shares no code with the library: tests
take their reference masks from here, so a change to the mixer, the pair / half selection or the
threshold moves the kernels away from it instead of moving the reference along."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_M64 = (1 << 64) - 1


def mix32(x):
    """lowbias32 on the low 32 bits of a uint64 array (or scalar)."""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def _ctrs(ctr):
    if isinstance(ctr, (int, np.integer)):
        return np.array([int(ctr) & _M64], dtype=np.uint64)
    return np.asarray(ctr, dtype=np.uint64)


def u16(seed, ctr):
    """The 16-bit draw of counter(s) ``ctr`` under the 64-bit ``seed`` (uint64 array, values < 65536)."""
    seed = int(seed) & _M64
    ctr = _ctrs(ctr)
    pair = ctr >> np.uint64(1)
    s = np.uint64(seed & 0xFFFFFFFF) ^ mix32(np.uint64(((seed >> 32) + 0x9E3779B9) & 0xFFFFFFFF))
    h = mix32((pair & _M32) ^ mix32((pair >> np.uint64(32)) ^ s))
    return np.where((ctr & np.uint64(1)) != 0, h >> np.uint64(16), h & np.uint64(0xFFFF))


def thresh(p):
    """Drop threshold on the 16-bit draw; ``p`` crosses the C ABI as a float."""
    p = np.float32(p)
    if p <= 0:
        return 0
    return min(65536, max(1, int(float(p) * 65536.0 + 0.5)))


def counters(offset, n):
    """offset, offset + 1, ... (n of them), modulo 2^64."""
    offset = int(offset) & _M64
    return np.uint64(offset) + np.arange(n, dtype=np.uint64)


def keep(seed, offset, n, p):
    """bool[n]: element i of a dropout site at counter ``offset`` is kept."""
    return u16(seed, counters(offset, n)) >= np.uint64(thresh(p))
