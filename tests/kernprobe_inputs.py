"""Seeded inputs and plain references for the kernel probe (tests/kernprobe/, tests/test_kernprobe_cpu.py, tests/test_kernprobe_gpu.py).

One builder per primitive of csrc/f3ds_kernels.inc returns a list of Case objects: a name, the edge classes the case belongs to, and its
arguments.  REQUIRED[primitive] lists the edge classes that have to be populated (the CPU test checks that none is empty).  Next to every
builder: ref_*(), the plain numpy reference the GPU result is compared with word for word, and slow_*(), a second formulation as a Python
loop that the CPU test holds against ref_*() on every case."""
import numpy as np

U32 = np.uint32
U64 = np.uint64
F = np.float32
NONE = 0xFFFFFFFF
HT_CAP = 256
SCAN_TILE = 2048
RS_TILE = 4096
RS_MAXBITS = 9
RL_LDS_CAP = 12288
QL = 64
NO_LABEL = 0xFFFFFFFF
EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)
NRANDOM = 200          # seeded random cases per wave-level primitive


class Case:
    def __init__(self, name, classes, **kw):
        self.name = name
        self.classes = set([classes] if isinstance(classes, str) else classes)
        self.__dict__.update(kw)

    def __repr__(self):
        return "Case(%s)" % self.name


def classes_of(cases):
    out = {}
    for c in cases:
        for k in c.classes:
            out.setdefault(k, []).append(c.name)
    return out


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64) & 0xFFFFFFFF, U32) if not (isinstance(a, np.ndarray) and a.dtype == U32) else np.ascontiguousarray(a)


def _rand32(rng, n, small=False):
    if small:
        return rng.integers(0, 1000, n, dtype=np.int64).astype(U32)
    return rng.integers(0, 1 << 32, n, dtype=np.int64).astype(U32)


# ---- scans over a wave / a workgroup ------------------------------------------------------------------------------------------------------
def scan_cases(width):
    """width 64 (wave_incl_scan, wave_incl_scan_dpp) or 256 (block_incl_scan<256>; block_excl_scan2 takes v and v2)"""
    rng = np.random.default_rng(1000 + width)
    out = [Case("all zero", "all zero", v=np.zeros(width, U32)), Case("all 0xFFFFFFFF", "all 0xFFFFFFFF (wraps)", v=np.full(width, NONE, U32))]
    at = list(EDGE_LANES) + ([64, 255, 127, 128, 191, 192] if width == 256 else [])
    for l in at:
        v = np.zeros(width, U32); v[l] = 1
        out.append(Case("single 1 at %d" % l, "single 1 at %s %d" % ("lane" if l < 64 else "thread", l), v=v))
    for i in range(NRANDOM):
        small = i % 3 == 0
        out.append(Case("random %d" % i, "random" if small else ["random", "random (wraps)"], v=_rand32(rng, width, small)))
    for c in out:
        c.v2 = np.roll(c.v, 7) ^ U32(0x5A5A5A5A) if "random" in c.classes else c.v[::-1].copy()
    return out


REQUIRED = {}
REQUIRED["scan64"] = ["all zero", "all 0xFFFFFFFF (wraps)", "random"] + ["single 1 at lane %d" % l for l in EDGE_LANES]
REQUIRED["scan256"] = REQUIRED["scan64"] + ["single 1 at thread %d" % t for t in (64, 255)]      # (thread 63 = lane 63)


def ref_incl_scan(v):
    return np.cumsum(v.astype(U32), dtype=U32)


def slow_incl_scan(v):
    out, run = [], 0
    for x in v.tolist():
        run = (run + x) & 0xFFFFFFFF
        out.append(run)
    return np.array(out, U32)


def ref_excl_scan(v):
    return (ref_incl_scan(v) - v.astype(U32)).astype(U32)


# ---- minima and the 16-lane sort ----------------------------------------------------------------------------------------------------------
def minsort_cases():
    rng = np.random.default_rng(2000)
    out = []
    for l in range(64):
        v = rng.integers(1000, 1 << 32, 64, dtype=np.int64).astype(U32); v[l] = U32(rng.integers(0, 1000))
        out.append(Case("minimum at lane %d" % l, "minimum at lane %d" % l, v=v))
    out.append(Case("all equal", "all equal", v=np.full(64, 0x12345678, U32)))
    out.append(Case("all equal, bit 31", ["all equal", "bit 31 set"], v=np.full(64, 0x80000001, U32)))
    for i in range(8):
        v = rng.integers(0, 1 << 31, 64, dtype=np.int64).astype(U32)
        hi = rng.random(64) < 0.5
        v[hi] |= U32(0x80000000)
        if i == 0:
            v[:] |= U32(0x80000000)
        out.append(Case("bit 31 mix %d" % i, "bit 31 set", v=v))
    asc = np.arange(64, dtype=np.int64) * 3 + 5
    out.append(Case("ascending", "ascending", v=u32(asc)))
    out.append(Case("descending", "descending", v=u32(asc[::-1])))
    out.append(Case("descending rows, bit 31", ["descending", "bit 31 set"], v=u32(0xFFFFFF00 - asc)))
    out.append(Case("all 0xFFFFFFFF", "all 0xFFFFFFFF", v=np.full(64, NONE, U32)))
    for k in range(1, 16):
        v = np.full(64, NONE, U32)
        for r in range(4):
            real = rng.integers(0, 1 << 20, k, dtype=np.int64).astype(U32)
            if r & 1:
                v[16 * r:16 * r + k] = real                  # the first k lanes, as a helper's raw tile list sits
            else:
                v[16 * r + rng.permutation(16)[:k]] = real   # anywhere in the row
        out.append(Case("%d real entries padded" % k, "%d real entries padded with 0xFFFFFFFF" % k, v=v))
    for i in range(8):
        out.append(Case("heavy duplicates %d" % i, "heavy duplicates", v=rng.integers(0, 2 + i % 3, 64, dtype=np.int64).astype(U32) * U32(0x40000001)))
    v = np.concatenate([np.arange(16), np.arange(16)[::-1] + 100, rng.integers(0, 3, 16), np.r_[rng.integers(0, 1 << 32, 5, dtype=np.int64), np.full(11, NONE)]])
    out.append(Case("four different rows", "four different rows", v=u32(v)))
    for i in range(NRANDOM):
        out.append(Case("random %d" % i, "random", v=_rand32(rng, 64, i % 4 == 0)))
    return out


REQUIRED["minsort"] = (["minimum at lane %d" % l for l in range(64)] + ["all equal", "bit 31 set", "ascending", "descending", "all 0xFFFFFFFF", "heavy duplicates",
                       "four different rows", "random"] + ["%d real entries padded with 0xFFFFFFFF" % k for k in range(1, 16)])


def ref_wave_min(v):
    return np.full(64, v.min(), U32)


def ref_row_min(v):
    return np.repeat(v.reshape(4, 16).min(1), 16).astype(U32)


def ref_row_sort(v):
    return np.sort(v.reshape(4, 16), axis=1).reshape(64)


def slow_min(v, width):
    out = []
    for l in range(64):
        b = l // width * width
        m = v[b]
        for x in v[b:b + width].tolist():
            if x < m:
                m = x
        out.append(m)
    return np.array(out, U32)


def slow_row_sort(v):
    return np.array(sum((sorted(v[16 * r:16 * r + 16].tolist()) for r in range(4)), []), U32)


# ---- run_of_lane ----------------------------------------------------------------------------------------------------------------------------
def run_cases():
    rng = np.random.default_rng(3000)
    ones = np.ones(64, U32)
    out = [Case("one run over all lanes", "one run covering all 64 lanes", valid=ones.copy(), w0=np.full(64, 7, U32), w1=np.full(64, 9, U32))]
    for start in (1, 32, 48, 62, 63):
        w0 = np.arange(64, dtype=U32); w0[start:] = 1000
        out.append(Case("run %d..63" % start, "run ending at lane 63", valid=ones.copy(), w0=w0, w1=np.zeros(64, U32)))
    v = ones.copy(); v[10] = 0; v[63] = 0; v[0] = 0; v[31] = 0
    out.append(Case("invalid lane beside a valid lane with the same word", "invalid lane next to a valid lane holding the same word", valid=v, w0=np.full(64, 5, U32), w1=np.full(64, 5, U32)))
    v = ones.copy(); v[1::2] = 0
    out.append(Case("every other lane invalid, same word", "invalid lane next to a valid lane holding the same word", valid=v, w0=np.zeros(64, U32), w1=np.zeros(64, U32)))
    out.append(Case("alternating words", "alternating words", valid=ones.copy(), w0=u32(np.arange(64) & 1), w1=np.zeros(64, U32)))
    out.append(Case("alternating pairs", "alternating words", valid=ones.copy(), w0=u32((np.arange(64) >> 1) & 1), w1=np.zeros(64, U32)))
    out.append(Case("equal w0, w1 differs", "equal w0 with differing w1", valid=ones.copy(), w0=np.full(64, 3, U32), w1=u32(np.arange(64) // 5)))
    out.append(Case("equal w1, w0 differs", "equal w1 with differing w0", valid=ones.copy(), w0=u32(np.arange(64) // 7), w1=np.full(64, NONE, U32)))
    out.append(Case("nothing valid", "nothing valid", valid=np.zeros(64, U32), w0=np.zeros(64, U32), w1=np.zeros(64, U32)))
    for i in range(NRANDOM):
        runs = np.cumsum(rng.random(64) < rng.choice([0.1, 0.3, 0.7]))
        valid = (rng.random(64) < rng.choice([1.0, 0.9, 0.5])).astype(U32)
        two = rng.random() < 0.5
        out.append(Case("random %d" % i, "random", valid=valid, w0=u32(runs if not two else runs // 2), w1=u32(runs & 1 if two else 0 * runs)))
    return out


REQUIRED["run_of_lane"] = ["one run covering all 64 lanes", "run ending at lane 63", "invalid lane next to a valid lane holding the same word", "alternating words",
                           "equal w0 with differing w1", "random"]


def ref_run_of_lane(valid, w0, w1):
    """(head, head_lane, run_len) per lane; head_lane and run_len are defined for valid lanes (0 elsewhere here)"""
    head = np.zeros(64, U32); hl = np.zeros(64, U32); ln = np.zeros(64, U32)
    for l in range(64):
        head[l] = valid[l] and (l == 0 or not valid[l - 1] or w0[l - 1] != w0[l] or w1[l - 1] != w1[l])
    for l in range(64):
        if not valid[l]:
            continue
        a = l
        while not head[a]:
            a -= 1
        b = a + 1
        while b < 64 and valid[b] and not head[b]:
            b += 1
        hl[l] = a; ln[l] = b - a
    return head, hl, ln


def slow_run_of_lane(valid, w0, w1):
    head = np.zeros(64, U32); hl = np.zeros(64, U32); ln = np.zeros(64, U32)
    same = lambda a, b: valid[a] and valid[b] and w0[a] == w0[b] and w1[a] == w1[b]
    for l in range(64):
        if not valid[l]:
            continue
        a = l
        while a > 0 and same(a - 1, a):
            a -= 1
        b = l
        while b < 63 and same(b, b + 1):
            b += 1
        head[l] = a == l; hl[l] = a; ln[l] = b - a + 1
    return head, hl, ln


# ---- d_scan_single, scan_u32 ----------------------------------------------------------------------------------------------------------------
def scan_single_cases():
    rng = np.random.default_rng(4000)
    out = []
    for m in (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192 + 5):
        out.append(Case("m = %d" % m, "m = %d" % m, data=_rand32(rng, m, True)))
    for bits, nb in ((1, 1), (3, 1), (9, 1), (9, 2), (9, 3), (8, 5), (7, 9), (9, 17), (5, 33)):
        m = (1 << bits) * nb
        out.append(Case("(1 << %d) * %d" % (bits, nb), "the product's (1 << bits) * nb shapes", data=rng.integers(0, 4097, m, dtype=np.int64).astype(U32)))
    for m in (3, 4096, 4097, 10000):
        out.append(Case("total wraps, m = %d" % m, "total wraps", data=_rand32(rng, m)))
    out.append(Case("all 0xFFFFFFFF, m = 5000", "total wraps", data=np.full(5000, NONE, U32)))
    for i in range(40):
        out.append(Case("random %d" % i, "random", data=_rand32(rng, int(rng.integers(0, 13000)), i % 2 == 0)))
    return out


REQUIRED["scan_single"] = ["m = %d" % m for m in (0, 1, 15, 16, 17, 4095, 4096, 4097, 8197)] + ["the product's (1 << bits) * nb shapes", "total wraps", "random"]


def scan_u32_cases():
    rng = np.random.default_rng(5000)
    out = []
    for n in (0, 1, 2047, 2048, 2049, 3 * 2048, 5 * 2048 + 77):
        cl = ["n = %d" % n] + (["several tiles"] if n > 4096 else [])
        out.append(Case("n = %d" % n, cl, data=_rand32(rng, n, True), extra=0))
        out.append(Case("n = %d, launch 3 wider" % n, cl + ["launch wider than n needs"], data=_rand32(rng, n, True), extra=3))
    out.append(Case("wraps", ["total wraps", "several tiles"], data=_rand32(rng, 7000), extra=1))
    for i in range(30):
        out.append(Case("random %d" % i, "random", data=_rand32(rng, int(rng.integers(0, 20000)), i % 2 == 0), extra=int(rng.integers(0, 3))))
    return out


REQUIRED["scan_u32"] = ["n = %d" % n for n in (0, 1, 2047, 2048, 2049)] + ["several tiles", "launch wider than n needs", "random"]


# ---- radix sort -----------------------------------------------------------------------------------------------------------------------------
RADIX_N = (0, 1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 1)


def _radix_keys(rng, n, pattern, shift, bits):
    """keys whose digit (keys >> shift) & mask follows `pattern`; the bits around the digit are random (they must be ignored but carried along)"""
    mask = (1 << bits) - 1
    if pattern == "random":
        d = rng.integers(0, mask + 1, n)
    elif pattern == "all equal":
        d = np.full(n, int(rng.integers(0, mask + 1)))
    elif pattern == "sorted":
        d = np.sort(rng.integers(0, mask + 1, n))
    elif pattern == "reversed":
        d = np.sort(rng.integers(0, mask + 1, n))[::-1]
    elif pattern == "alternating":
        a, b = int(rng.integers(0, mask + 1)), int(rng.integers(0, mask + 1))
        d = np.where(np.arange(n) & 1, a, b if b != a or mask == 0 else a ^ 1)
    else:
        raise KeyError(pattern)
    noise = rng.integers(0, 1 << 62, n, dtype=np.int64).astype(U64) | (rng.integers(0, 4, n, dtype=np.int64).astype(U64) << U64(62))
    hole = ~(U64(mask) << U64(shift))
    return ((noise & hole) | (d.astype(U64) << U64(shift))).astype(U64)


def radix_pass_cases():
    """one pass: d_radix_hist, d_radix_scatter, d_radix_scatter_k.  idx > 0: the keys carry their index in their low idx bits (the _k flavour's payload)"""
    rng = np.random.default_rng(6000)
    out = []
    shifts = (0, 3, 17, 40, 55)
    i = 0
    for n in RADIX_N:
        for pattern in ("random", "all equal", "sorted", "reversed", "alternating"):
            if pattern != "random" and n not in (65, 4096, 4097, 3 * 4096 + 1):
                continue
            bits = 1 + i % RS_MAXBITS; shift = shifts[i % len(shifts)]; i += 1
            cl = ["n = %d" % n, "bits = %d" % bits, "shift = %d" % shift, pattern, "bits above the sorted range"]
            if pattern == "all equal" and n >= 4096:
                cl.append("one digit receives all 4096 keys of a tile")
            out.append(Case("n = %d, %s, bits %d, shift %d" % (n, pattern, bits, shift), cl, keys=_radix_keys(rng, n, pattern, shift, bits), shift=shift, bits=bits, n_dev=-1, idx=0))
    for bits in range(1, RS_MAXBITS + 1):
        for n in (4097, 300):
            shift = int(rng.integers(0, 56))
            out.append(Case("bits %d, n = %d, shift %d" % (bits, n, shift), ["bits = %d" % bits, "random"], keys=_radix_keys(rng, n, "random", shift, bits), shift=shift, bits=bits, n_dev=-1, idx=0))
    for n, nd in ((4097, 4096), (4097, 100), (9000, 4095), (65, 0), (5000, 6000)):
        out.append(Case("n_dev %d of n = %d" % (nd, n), "n_dev < n" if nd < n else "n_dev >= n", keys=_radix_keys(rng, n, "random", 5, 8), shift=5, bits=8, n_dev=nd, idx=0))
    for n, idx in ((1, 1), (64, 6), (4097, 13), (3 * 4096 + 1, 14)):
        for pattern in ("random", "alternating", "all equal"):
            bits = int(rng.integers(1, RS_MAXBITS + 1)); shift = idx + int(rng.integers(0, 20))
            k = _radix_keys(rng, n, pattern, shift, bits)
            k = (k & ~U64((1 << idx) - 1)) | np.arange(n, dtype=U64)
            out.append(Case("index in the low %d bits, n = %d, %s" % (idx, n, pattern), ["index in the low bits", pattern], keys=k, shift=shift, bits=bits, n_dev=-1, idx=idx))
    for c in out:
        c.vals = np.random.default_rng(len(c.keys)).permutation(len(c.keys)).astype(U32) ^ U32(0xA5000000)
    return out


REQUIRED["radix_pass"] = (["n = %d" % n for n in RADIX_N] + ["bits = %d" % b for b in range(1, 10)] + ["shift = 55", "all equal", "sorted", "reversed", "alternating", "random",
                          "n_dev < n", "bits above the sorted range", "index in the low bits", "one digit receives all 4096 keys of a tile"])


def radix_nb(n):
    return (n + RS_TILE - 1) // RS_TILE if n else 1


def _n_eff(c):
    n = len(c.keys)
    return n if c.n_dev < 0 else min(n, c.n_dev)


def ref_radix_hist(c):
    """hist[d * nb + tile]"""
    n, ne, nb = len(c.keys), _n_eff(c), radix_nb(len(c.keys))
    d = ((c.keys[:ne] >> U64(c.shift)) & U64((1 << c.bits) - 1)).astype(np.int64)
    h = np.zeros(((1 << c.bits), nb), np.int64)
    for t in range(nb):
        h[:, t] = np.bincount(d[t * RS_TILE:(t + 1) * RS_TILE], minlength=1 << c.bits)
    return h.reshape(-1).astype(U32)


def slow_radix_hist(c):
    ne, nb = _n_eff(c), radix_nb(len(c.keys))
    h = [0] * ((1 << c.bits) * nb)
    for i, k in enumerate(c.keys[:ne].tolist()):
        h[((k >> c.shift) & ((1 << c.bits) - 1)) * nb + i // RS_TILE] += 1
    return np.array(h, U32)


def ref_radix_scatter(c):
    """stable partition by digit of the first n_eff pairs; what lies behind them stays zero"""
    n, ne = len(c.keys), _n_eff(c)
    d = ((c.keys[:ne] >> U64(c.shift)) & U64((1 << c.bits) - 1)).astype(np.int64)
    order = np.argsort(d, kind="stable")
    ko = np.zeros(n, U64); vo = np.zeros(n, U32)
    ko[:ne] = c.keys[:ne][order]; vo[:ne] = c.vals[:ne][order]
    return ko, vo


def slow_radix_scatter(c):
    n, ne = len(c.keys), _n_eff(c)
    bins = [[] for _ in range(1 << c.bits)]
    for i, k in enumerate(c.keys[:ne].tolist()):
        bins[(k >> c.shift) & ((1 << c.bits) - 1)].append(i)
    order = np.array(sum(bins, []), np.int64)
    ko = np.zeros(n, U64); vo = np.zeros(n, U32)
    ko[:ne] = c.keys[:ne][order]; vo[:ne] = c.vals[:ne][order]
    return ko, vo


def radix_sort_cases():
    rng = np.random.default_rng(7000)
    out = []
    for n in RADIX_N + (20000,):
        for total, base in ((25, 0), (10, 0), (9, 14), (33, 0), (1, 3), (19, 14), (0, 0)):
            if n > 4097 and total in (1, 0):
                continue
            k = rng.integers(0, 1 << 62, n, dtype=np.int64).astype(U64)
            if total and (n + total) % 3 == 0:          # few distinct digits: long runs of equal keys, stability shows
                k = (k & ~(U64((1 << total) - 1) << U64(base))) | (rng.integers(0, 3, n, dtype=np.int64).astype(U64) << U64(base + total - 1) >> U64(1) << U64(1))
            cl = ["n = %d" % n, "total_bits = %d" % total] + (["base_shift > 0"] if base else []) + ["bits above the sorted range"]
            out.append(Case("n = %d, %d bits from %d" % (n, total, base), cl, keys=k, total=total, base=base, n_dev=-1, pairs=True))
            out.append(Case("n = %d, %d bits from %d, keys only" % (n, total, base), cl + ["keys only"], keys=k, total=total, base=base, n_dev=-1, pairs=False))
    for n, nd, total in ((4097, 4000, 25), (9000, 4096, 18), (9000, 1, 9), (300, 0, 12)):
        k = rng.integers(0, 1 << 62, n, dtype=np.int64).astype(U64)
        out.append(Case("n_dev %d of %d, %d bits" % (nd, n, total), "n_dev < n", keys=k, total=total, base=14, n_dev=nd, pairs=True))
    for name, k in (("all keys equal", np.full(5000, 0x123456789, U64)), ("already sorted", np.sort(rng.integers(0, 1 << 25, 5000, dtype=np.int64)).astype(U64)),
                    ("reversed", np.sort(rng.integers(0, 1 << 25, 5000, dtype=np.int64))[::-1].astype(U64)), ("two values alternating", np.where(np.arange(5000) & 1, 77, 3).astype(U64))):
        out.append(Case(name, name, keys=np.ascontiguousarray(k), total=25, base=0, n_dev=-1, pairs=True))
        out.append(Case(name + ", keys only", [name, "keys only"], keys=np.ascontiguousarray(k), total=25, base=0, n_dev=-1, pairs=False))
    for c in out:
        c.vals = np.arange(len(c.keys), dtype=U32)[::-1].copy()
    return out


REQUIRED["radix_sort"] = ["n = %d" % n for n in RADIX_N] + ["base_shift > 0", "n_dev < n", "keys only", "all keys equal", "already sorted", "reversed", "two values alternating",
                                                             "bits above the sorted range"]


def radix_passes(total):
    """the (shift, bits) of radix_sort's passes"""
    if total <= 0:
        return []
    passes = (total + RS_MAXBITS - 1) // RS_MAXBITS
    per = (total + passes - 1) // passes
    out, shift = [], 0
    for _ in range(passes):
        bits = min(per, total - shift)
        out.append((shift, bits)); shift += bits
    return out


def ref_radix_sort(c):
    """np.argsort(kind="stable") on the masked bits of the first n_eff keys.  Behind them: the buffer the last pass wrote to was zero there, the other
    one still holds the input (an even number of passes ends in the input's buffer)"""
    n, ne = len(c.keys), _n_eff(c)
    np_ = len(radix_passes(c.total))
    d = (c.keys[:ne] >> U64(c.base)) & U64((1 << c.total) - 1)
    order = np.argsort(d, kind="stable")
    ko = c.keys.copy() if np_ % 2 == 0 else np.zeros(n, U64)
    vo = c.vals.copy() if np_ % 2 == 0 else np.zeros(n, U32)
    ko[:ne] = c.keys[:ne][order]; vo[:ne] = c.vals[:ne][order]
    return ko, vo


def slow_radix_sort(c):
    """LSD passes of the slow one-pass formulation"""
    n, ne = len(c.keys), _n_eff(c)
    k, v = c.keys.copy(), c.vals.copy()
    k2, v2 = np.zeros(n, U64), np.zeros(n, U32)
    for shift, bits in radix_passes(c.total):
        o = slow_radix_scatter(Case("pass", "pass", keys=k, vals=v, shift=c.base + shift, bits=bits, n_dev=c.n_dev))
        k2[:ne] = o[0][:ne]; v2[:ne] = o[1][:ne]
        k, k2, v, v2 = k2, k, v2, v
    return k, v


# ---- the segment table ------------------------------------------------------------------------------------------------------------------------
def seg_cases():
    rng = np.random.default_rng(8000)
    out = []

    def add(name, cl, codes, limit, shift):
        codes = np.asarray(codes, np.int64)
        assert (np.diff(codes) >= 0).all()
        low = rng.integers(0, 1 << shift, len(codes), dtype=np.int64) if shift else 0
        out.append(Case(name, list(cl) + ["shift = 0" if shift == 0 else "shift > 0"], keys=((codes << shift) | low).astype(U64), limit=int(limit), shift=shift))

    for shift in (0, 13):
        s = ", shift %d" % shift
        add("n = 0" + s, ["n = 0"], [], 100, shift)
        add("no valid key" + s, ["no valid key"], np.sort(rng.integers(100, 200, 5000)), 100, shift)
        add("one invalid key" + s, ["no valid key"], [100], 100, shift)
        add("all valid and distinct" + s, ["all keys valid and distinct"], np.arange(6000) * 2, 1 << 40, shift)
        add("all keys equal" + s, ["all keys equal"], np.full(4500, 17), 18, shift)
        add("one valid key" + s, ["all keys equal", "all keys valid and distinct"], [5], 6, shift)
        for n in (2049, 4096 + 9, 10000):
            for what, every in (("a thread's first item", 8), ("a tile boundary", 2048)):
                codes = np.arange(n) // every
                add("boundaries at every %d, n = %d%s" % (every, n, s), ["segment boundary at " + what], codes, 1 << 30, shift)
            codes = np.zeros(n, np.int64); codes[n - 1] = 1
            add("boundary at n - 1, n = %d%s" % (n, s), ["segment boundary at n - 1"], codes, 5, shift)
            codes = np.sort(rng.integers(0, 50, n)); nv = int(rng.integers(1, n)); codes[nv:] = 1000
            add("invalid tail from %d, n = %d%s" % (nv, n, s), ["invalid keys only at the tail"], codes, 1000, shift)
        for nv in (8, 2048, 4096):
            codes = np.r_[np.arange(nv) // 3, np.full(300, 1 << 20)]
            add("valid keys end at %d%s" % (nv, s), ["invalid keys only at the tail", "valid keys end at a boundary of the launch"], codes, 1 << 20, shift)
    for i in range(60):
        n = int(rng.integers(1, 12000)); hi = int(rng.choice([3, 100, 100000]))
        codes = np.sort(rng.integers(0, hi, n)); limit = int(rng.integers(1, hi + 2))
        add("random %d" % i, ["random"], codes, limit, int(rng.choice([0, 0, 5, 20])))
    return out


REQUIRED["seg_table"] = ["no valid key", "all keys valid and distinct", "all keys equal", "segment boundary at a thread's first item", "segment boundary at a tile boundary",
                         "segment boundary at n - 1", "invalid keys only at the tail", "shift = 0", "shift > 0", "random"]


def ref_seg_table(c):
    """seg_start[n + 1] (zero behind the table) and (segments, valid keys)"""
    n = len(c.keys)
    k = c.keys >> U64(c.shift)
    valid = k < U64(c.limit)
    seg = np.zeros(n + 1, U32)
    if not valid.any():
        return seg, np.zeros(2, U32)
    nv = int(np.flatnonzero(valid)[-1]) + 1
    _, first = np.unique(k[:nv], return_index=True)
    seg[:len(first)] = first; seg[len(first)] = nv
    return seg, np.array([len(first), nv], U32)


def slow_seg_table(c):
    n = len(c.keys)
    seg = [0] * (n + 1); ns = nv = 0
    ks = [x >> c.shift for x in c.keys.tolist()]
    for i in range(n):
        if ks[i] >= c.limit:
            continue
        if i == 0 or ks[i - 1] != ks[i]:
            seg[ns] = i; ns += 1
        nv = i + 1
    if nv:
        seg[ns] = nv
    return np.array(seg, U32), np.array([ns, nv], U32)


# ---- relabel ----------------------------------------------------------------------------------------------------------------------------------
RELABEL_S0 = (1, 63, 64, 255, 256, 257, 1000)


def relabel_cases():
    rng = np.random.default_rng(9000)
    out = []

    def make(S0, kind, tag=""):
        parent = np.arange(S0 + 1, dtype=np.int64)
        if kind == "everybody alive" or kind == "nobody alive":
            alive = np.full(S0 + 1, kind == "everybody alive")
        else:
            depth = {"chains of length 1": 1, "chains of length 2": 2, "chains of about 50": 50, "random": int(rng.integers(1, 8))}[kind]
            nroots = max(1, S0 // (depth + 1)) if kind != "random" else max(1, int(rng.integers(1, S0 + 1)))
            labels = rng.permutation(S0) + 1
            roots = labels[:nroots]
            level = {0: list(roots)}
            rest = labels[nroots:]
            d = 1
            while len(rest):                                      # level d hangs off level d - 1: chains of `depth` links (the last level takes what is left)
                take = len(rest) if d >= depth else max(1, len(rest) // (depth - d + 1))
                level[d] = list(rest[:take])
                for h in level[d]:
                    parent[h] = level[d - 1][int(rng.integers(0, len(level[d - 1])))]
                rest = rest[take:]; d += 1
            alive = np.zeros(S0 + 1, bool)
            alive[roots] = rng.random(nroots) < 0.8          # (a root that never lived: its members get no label)
        alive[0] = bool(rng.integers(0, 2))                    # label 0 is nobody's, whatever its flag says
        V = int(rng.integers(1, 4 * S0 + 2))
        for n in ((0, 1, 255, 256, 257, 5000, 70000) if kind == "random" and S0 in (1, 257) else (int(rng.integers(1, 9000)),)):
            owner = rng.integers(0, S0 + 1, V); owner[rng.random(V) < 0.1] = 0
            pv = rng.integers(0, V, n); pv[rng.random(n) < 0.1] = -1
            if n > 2:
                owner[0] = 0; pv[0] = 0; pv[1] = -1
            cl = ["S0 = %d" % S0, kind, "n = %d" % n] + (["pt_voxel < 0", "owner 0"] if n > 2 else [])
            out.append(Case("S0 = %d, %s, n = %d%s" % (S0, kind, n, tag), cl, S0=S0, parent=u32(parent), ralive=alive.astype(np.uint8) * np.uint8(1 + (S0 & 1) * 254),
                            pt_voxel=np.ascontiguousarray(pv, np.int32), owner=u32(owner), V=V))

    for S0 in RELABEL_S0 + (3000,):
        for kind in ("nobody alive", "everybody alive", "chains of length 1", "chains of length 2", "chains of about 50", "random"):
            make(S0, kind)
    for i in range(200):
        make(int(rng.integers(1, 1500)), "random", ", %d" % i)
    return out


REQUIRED["relabel"] = ["S0 = %d" % s for s in RELABEL_S0] + ["nobody alive", "everybody alive", "chains of length 1", "chains of length 2", "chains of about 50", "pt_voxel < 0", "owner 0", "random"]


def ref_relabel(c):
    """(rank, root, incl, n_regions, labels)"""
    S0 = c.S0
    alive = c.ralive != 0
    alive[0] = False
    incl = np.cumsum(alive).astype(U32)
    root = np.arange(S0 + 1)
    while True:
        nxt = c.parent[root].astype(np.int64)
        if (nxt == root).all():
            break
        root = nxt
    rank = np.where(alive, incl - U32(1), U32(NO_LABEL)).astype(U32)
    rank = rank[root]
    o = c.owner[np.maximum(c.pt_voxel, 0)]
    labels = np.where((c.pt_voxel >= 0) & (o != 0), rank[o], U32(NO_LABEL)).astype(U32)
    return rank, root.astype(U32), incl, int(alive.sum()), labels


def slow_relabel(c):
    S0 = c.S0
    ids, nxt = {}, 0
    for h in range(1, S0 + 1):
        if c.ralive[h]:
            ids[h] = nxt; nxt += 1
    rank, root, incl, run = [], [], [], 0
    for h in range(S0 + 1):
        r = h
        while int(c.parent[r]) != r:
            r = int(c.parent[r])
        root.append(r); rank.append(ids.get(r, NO_LABEL))
        run += 1 if h in ids else 0
        incl.append(run)
    labels = []
    for v in c.pt_voxel.tolist():
        labels.append(rank[int(c.owner[v])] if v >= 0 and c.owner[v] != 0 else NO_LABEL)
    return np.array(rank, U32), np.array(root, U32), np.array(incl, U32), nxt, np.array(labels, U32)


# ---- helper_tile_list -------------------------------------------------------------------------------------------------------------------------
def tile_list_cases():
    rng = np.random.default_rng(10000)
    out = []

    def add(name, cl, raw, gv):
        tl = rng.integers(0, 1 << 20, HT_CAP, dtype=np.int64)          # (what lies behind the list must not be read as part of it)
        raw = np.asarray(raw, np.int64)
        tl[:min(len(raw), HT_CAP)] = raw[:HT_CAP]
        out.append(Case(name, cl, tl=u32(tl), cnt=len(raw), gv=int(gv)))

    def raw_of(n, distinct):
        pool = rng.choice(1 << 20, distinct, replace=False)
        raw = np.r_[pool, pool[rng.integers(0, distinct, n - distinct)]] if n >= distinct else pool[:n]
        return raw[rng.permutation(len(raw))]

    for cnt in (0, 1, 2, 15, 16, 17, 63, 64):
        for distinct in sorted({cnt, max(1, cnt // 2), 1} if cnt else {0}):
            raw = raw_of(cnt, distinct) if cnt else np.zeros(0, np.int64)
            base = ["cnt = %d" % cnt]
            add("cnt %d, %d distinct, no ghost" % (cnt, distinct), base + ["no ghost"], raw, -1)
            new = int(rng.integers(1 << 20, 1 << 21))
            add("cnt %d, %d distinct, ghost in a new tile" % (cnt, distinct), base + ["ghost tile new"] + (["64 plus a ghost: multi-round path"] if cnt == 64 else []), raw, new * 64 + int(rng.integers(0, 64)))
            if cnt:
                add("cnt %d, %d distinct, ghost in a listed tile" % (cnt, distinct), base + ["ghost tile equal to a listed tile"] + (["64 plus a ghost: multi-round path"] if cnt == 64 else []),
                    raw, int(raw[int(rng.integers(0, cnt))]) * 64 + int(rng.integers(0, 64)))
    for n in (65, 128, 256):
        for distinct in (1, 63, 64, 65):
            raw = raw_of(n, distinct)
            cl = ["%d raw entries" % n, "%d distinct tiles" % distinct] + (["more than 64 distinct tiles: -1"] if distinct > 64 else [])
            add("%d raw, %d distinct" % (n, distinct), cl + ["no ghost"], raw, -1)
            add("%d raw, %d distinct, ghost listed" % (n, distinct), cl + ["ghost tile equal to a listed tile"], raw, int(raw[0]) * 64 + 63)
            add("%d raw, %d distinct, ghost new" % (n, distinct), cl + ["ghost tile new"] + (["the ghost is the 65th distinct tile: -1"] if distinct == 64 else []), raw, (1 << 26) + 5)
    add("cnt = HT_CAP + 1", ["cnt = HT_CAP + 1 gives -1"], np.arange(HT_CAP + 1), -1)
    add("cnt = HT_CAP + 1, ghost", ["cnt = HT_CAP + 1 gives -1"], np.zeros(HT_CAP + 1), 64)
    for i in range(300):
        n = int(rng.integers(0, HT_CAP + 1)) if i % 2 else int(rng.integers(0, 65))
        distinct = int(rng.integers(1, min(n, 70) + 1)) if n else 0
        add("random %d" % i, ["random"], raw_of(n, distinct) if n else [], -1 if rng.random() < 0.5 else int(rng.integers(0, 1 << 26)))
    return out


REQUIRED["tile_list"] = (["cnt = %d" % c for c in (0, 1, 63, 64)] + ["no ghost", "ghost tile new", "ghost tile equal to a listed tile", "64 plus a ghost: multi-round path"]
                         + ["%d raw entries" % n for n in (65, 128, 256)] + ["%d distinct tiles" % d for d in (1, 63, 64, 65)]
                         + ["more than 64 distinct tiles: -1", "the ghost is the 65th distinct tile: -1", "cnt = HT_CAP + 1 gives -1", "random"])


def ref_tile_list(tl, cnt, gv):
    """sorted distinct tiles, or None for -1"""
    if cnt > HT_CAP:
        return None
    s = set(tl[:cnt].tolist()) | ({gv >> 6} if gv >= 0 else set())
    return None if len(s) > 64 else sorted(s)


def slow_tile_list(tl, cnt, gv):
    if cnt > HT_CAP:
        return None
    seen = []
    for x in tl[:cnt].tolist() + ([gv >> 6] if gv >= 0 else []):
        if x not in seen:
            seen.append(x)
    if len(seen) > 64:
        return None
    for i in range(len(seen)):                       # selection sort
        j = min(range(i, len(seen)), key=lambda q: seen[q])
        seen[i], seen[j] = seen[j], seen[i]
    return seen


# ---- row_leaves -------------------------------------------------------------------------------------------------------------------------------
def _row_state(rng, V, h, nd, leaves_target, owner, free_tiles, dup=True):
    """a helper h with nd distinct listed tiles (taken from free_tiles) and about leaves_target owned voxels in them; returns its raw list (<= 16 entries)"""
    tiles = [free_tiles.pop() for _ in range(nd)]
    raw = list(tiles)
    while dup and len(raw) < 16 and raw and rng.random() < 0.5:
        raw.append(raw[int(rng.integers(0, len(raw)))])
    raw = [raw[i] for i in rng.permutation(len(raw))]
    vox = np.concatenate([np.arange(t * 64, min(t * 64 + 64, V)) for t in tiles]) if tiles else np.zeros(0, np.int64)
    pick = rng.permutation(len(vox))[:min(leaves_target, len(vox))]
    owner[vox[pick]] = h
    return raw


def row_leaves_cases():
    rng = np.random.default_rng(11000)
    out = []

    def new_case(name, cl, V, rows, cap=QL):
        """rows: four of (nd, leaves_target, ghost) with ghost in None | ("bit", b) | "unowned tile" | "outside" """
        T = (V + 63) // 64
        owner = rng.integers(100, 200, V)
        free = list(rng.permutation(T))
        hs, tids, gvs = [], np.full(64, NONE, np.int64), []
        cl = list(cl)
        for r, (nd, target, ghost) in enumerate(rows):
            h = 0 if nd is None else r + 1 + 4 * int(rng.integers(0, 5))
            nd = nd or 0
            want_last = V % 64 and nd and (T - 1) in free and r == 0
            if want_last:
                free.remove(T - 1); free.append(T - 1); cl.append("V not a multiple of 64 with the last tile listed")
            raw = _row_state(rng, V, h, min(nd, len(free)), target, owner, free, dup=ghost is None)
            gv = -1
            if ghost is not None and ghost != "outside" and (len(raw) >= 16 or not free):
                ghost = None
            if ghost == "outside" and free:
                gv = int(free.pop()) * 64; cl.append("ghost outside every listed tile")
            elif isinstance(ghost, tuple):
                t = int(raw[0]) if raw and rng.random() < 0.7 else None
                if t is None:
                    t = int(free.pop()); raw.append(t)
                g = t * 64 + ghost[1]
                if g < V:
                    gv = g; cl.append("ghost at tile bit %d" % ghost[1])
                    if t == T - 1 and V % 64:
                        cl.append("ghost in the last, partial tile")
            elif ghost == "unowned tile":
                t = int(free.pop()); raw.append(t); gv = t * 64 + int(rng.integers(0, min(64, V - t * 64)))
                cl.append("ghost in a tile the helper owns nothing in")
            tids[16 * r:16 * r + len(raw)] = raw
            hs.append(h); gvs.append(gv)
        c = Case(name, cl, V=V, owner=u32(owner), hs=u32(hs), tids=u32(tids), gvs=np.array(gvs, np.int32), cap=cap)
        for r in range(4):
            n = ref_row_leaves(c)[r][1]
            nd_ = len(ref_row_leaves(c)[r][0])
            c.classes.add("%d distinct tiles" % nd_)
            c.classes.add("%d list entries" % int((c.tids[16 * r:16 * r + 16] != NONE).sum()))
            if n in (63, 64):
                c.classes.add("%d leaves" % n)
            elif 65 <= n <= 100:
                c.classes.add("65..100 leaves")
        out.append(c)

    for nd in range(0, 17):
        new_case("nd %d in every row" % nd, ["list with duplicates"], 64 * 80 + 37, [(nd, 20, None)] * 4)
    new_case("rows of 0, 16, 3, 9 distinct tiles", ["four rows with different nd"], 64 * 90 + 1, [(0, 0, None), (16, 40, None), (3, 64, None), (9, 9, None)])
    new_case("rows of 16, none, 1, 0", ["four rows with different nd", "a row without a helper"], 64 * 40 + 63, [(16, 64, None), (None, 0, None), (1, 64, None), (0, 0, None)])
    for b in (0, 15, 16, 31, 32, 63):
        new_case("ghost at bit %d" % b, [], 64 * 50 + 64 * (b == 63) + 33 * (b != 63), [(3, 30, ("bit", b)), (1, 5, ("bit", b)), (7, 64, ("bit", b)), (0, 0, ("bit", b))])
    new_case("ghost in the last tile", [], 64 * 3 + 17, [(1, 10, ("bit", 15)), (1, 5, ("bit", 16)), (1, 3, ("bit", 0)), (0, 0, None)])
    new_case("ghost in an unowned tile", [], 64 * 30 + 5, [(2, 10, "unowned tile"), (0, 0, "unowned tile"), (15, 30, "unowned tile"), (4, 64, None)])
    new_case("ghost outside the list", [], 64 * 30 + 5, [(2, 10, "outside"), (0, 0, "outside"), (16, 30, "outside"), (4, 64, None)])
    for n in (63, 64, 65, 66, 80, 100):
        new_case("%d leaves" % n, ["truncated at cap" if n > 64 else "fits"], 64 * 64, [(2, n, None), (4, n, None), (16, n, None), (3, 10, None)])
        new_case("%d leaves, one tile full" % n, ["truncated at cap" if n > 64 else "fits"], 64 * 20, [(1, 64, None), (2, n, ("bit", 0)), (5, n, None), (2, 128, None)])
    new_case("cap 16", ["cap below QL"], 64 * 20, [(2, 16, None), (2, 17, None), (3, 15, None), (1, 64, None)], cap=16)
    new_case("V = 1", ["V = 1"], 1, [(1, 1, None), (0, 0, None), (0, 0, None), (0, 0, None)])
    for i in range(250):
        V = int(rng.integers(1, 64 * 70))
        ghosts = [None, None, ("bit", int(rng.integers(0, 64))), ("bit", int(rng.integers(0, 64))), "unowned tile", "outside"]
        rows = [(int(rng.integers(0, 17)) if rng.random() < 0.9 else None, int(rng.choice([0, 3, 20, 64, 90])), ghosts[int(rng.integers(0, 6))]) for _ in range(4)]
        new_case("random %d" % i, ["random"], V, rows)
    return out


REQUIRED["row_leaves"] = (["%d list entries" % n for n in range(0, 17)] + ["list with duplicates", "four rows with different nd", "0 distinct tiles", "16 distinct tiles",
                          "V not a multiple of 64 with the last tile listed"] + ["ghost at tile bit %d" % b for b in (0, 15, 16, 31, 32, 63)]
                          + ["ghost in a tile the helper owns nothing in", "ghost outside every listed tile", "ghost in the last, partial tile", "63 leaves", "64 leaves", "65..100 leaves", "random"])


def ref_row_leaves(c):
    """per row: (distinct tiles ascending, number of leaves, leaves ascending, kept bits)"""
    out = []
    for r in range(4):
        t = c.tids[16 * r:16 * r + 16]
        tiles = np.unique(t[t != NONE]).astype(np.int64)
        h, gv = int(c.hs[r]), int(c.gvs[r])
        leaves, kept = [], 0
        for i, tile in enumerate(tiles):
            v = np.arange(tile * 64, min(tile * 64 + 64, c.V))
            own = c.owner[v] == h
            if own.any():
                kept |= 1 << i
            leaves.append(v[own | (v == gv)])
        leaves = np.concatenate(leaves) if leaves else np.zeros(0, np.int64)
        out.append((tiles, len(leaves), leaves, kept))
    return out


def slow_row_leaves(c):
    out = []
    for r in range(4):
        tiles = []
        for x in c.tids[16 * r:16 * r + 16].tolist():
            if x != NONE and x not in tiles:
                tiles.append(x)
        tiles.sort()
        h, gv = int(c.hs[r]), int(c.gvs[r])
        leaves, kept = [], 0
        for i, tile in enumerate(tiles):
            for b in range(64):
                v = tile * 64 + b
                if v >= c.V:
                    break
                if c.owner[v] == h:
                    kept |= 1 << i
                if c.owner[v] == h or v == gv:
                    leaves.append(v)
        out.append((np.array(tiles, np.int64), len(leaves), np.array(leaves, np.int64), kept))
    return out


# ---- f3ds_vblock ------------------------------------------------------------------------------------------------------------------------------
VBLOCK_NF = (1, 7, 8, 9, 16, 17, 64)
VBLOCK_GX = (1, 2, 3, 5, 32)


# ---- d_centroid -------------------------------------------------------------------------------------------------------------------------------
class HelperState:
    """the books d_centroid reads and writes, for labels 0..S0 of one frame"""

    def __init__(self, S0, V):
        self.S0, self.V = S0, V
        L = S0 + 1
        self.owner = np.zeros(V, U32)
        self.vf = np.zeros((V, 12), F)
        self.ghost_active = np.zeros(L, np.uint8); self.ghost_done = np.zeros(L, np.uint8); self.ghost_vox = np.full(L, -1, np.int32)
        self.hlo = np.zeros(L, U32); self.hhi = np.zeros(L, U32); self.hcount = np.zeros(L, U32)
        self.tl = np.zeros((L, HT_CAP), U32); self.tcnt = np.zeros(L, U32)
        self.hc = np.zeros((L, 12), F)
        self.gx = 0

    def copy(self):
        o = HelperState.__new__(HelperState)
        for k, v in self.__dict__.items():
            o.__dict__[k] = v.copy() if isinstance(v, np.ndarray) else v
        return o

    def padded(self, V2, rng):
        """the same helpers in a frame of V2 >= V voxels: the added voxels are nobody's"""
        o = self.copy()
        o.V = V2
        o.owner = np.r_[self.owner, np.zeros(V2 - self.V, U32)]
        o.vf = np.concatenate([self.vf, _features(rng, V2 - self.V)])
        return o


def _features(rng, n):
    """V x 12 feature rows: xyz, rgb, a normal, three pad words (never read as data)"""
    vf = np.zeros((n, 12), F)
    vf[:, 0:3] = rng.uniform(-3, 3, (n, 3)); vf[:, 3:6] = rng.uniform(0, 255.99, (n, 3))
    nrm = rng.normal(size=(n, 3)); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)
    vf[:, 6:9] = nrm
    vf[:, 9:12] = rng.uniform(-1, 1, (n, 3))
    return vf


def centroid_states():
    """Cases of (name, classes, state) with V <= 48 * S0 (the row path); the GPU test runs each again padded to V > 48 * S0 (the wave path)"""
    rng = np.random.default_rng(12000)
    out = []

    def build(name, cl, S0, V, specs, gx=0):
        """specs[h - 1] = dict(tiles: distinct listed tiles holding leaves, leaves, stale: listed tiles without a leaf, raw: raw list length (duplicates fill up),
        ghost: None | "active" | "done" | "inactive" | "own" (the ghost voxel is the helper's), overflow: the list reads HT_CAP + 1)"""
        assert V <= 48 * S0 and len(specs) == S0
        st = HelperState(S0, V)
        st.vf = _features(rng, V)
        st.hc = rng.uniform(-1, 1, (S0 + 1, 12)).astype(F)
        st.gx = gx
        T = (V + 63) // 64
        cl = set(cl)
        tile_of = np.arange(V) >> 6
        for h, sp in enumerate(specs, 1):
            # helpers share tiles (V <= 48 * S0 leaves less than a tile per helper): a helper takes the emptiest of a random sample of tiles, and voxels nobody owns yet
            nfree = np.bincount(tile_of[st.owner == 0], minlength=T)
            nt = min(sp.get("tiles", 1), T)
            sample = rng.permutation(T)[:4 * nt + 8]
            tiles = [int(t) for t in sample[np.argsort(-nfree[sample], kind="stable")][:nt]]
            vox = np.flatnonzero(np.isin(tile_of, tiles) & (st.owner == 0))
            want = min(sp.get("leaves", 0), len(vox))
            mine = vox[rng.permutation(len(vox))[:want]]
            st.owner[mine] = h
            others = np.setdiff1d(np.arange(T), tiles)
            stale = [int(t) for t in others[rng.permutation(len(others))[:sp.get("stale", 0)]]]
            raw = tiles + stale
            while len(raw) < sp.get("raw", 0) and raw:
                raw.append(raw[int(rng.integers(0, len(raw)))])
            raw = [raw[i] for i in rng.permutation(len(raw))]
            g = sp.get("ghost")
            if g:
                if g == "own" and len(mine):
                    gv = int(mine[0])
                else:
                    cand = np.flatnonzero(st.owner != h)
                    gv = int(rng.choice(cand)) if len(cand) else -1
                if gv >= 0:
                    st.ghost_vox[h] = gv
                    st.ghost_active[h] = 0 if g == "inactive" else 1 + int(rng.integers(0, 2)) * 254
                    st.ghost_done[h] = 1 if g == "done" else 0
                    cl.add("ghost " + g)
            own_and_ghost = list(mine) + ([int(st.ghost_vox[h])] if st.ghost_vox[h] >= 0 else [])
            st.hlo[h] = min(own_and_ghost) if own_and_ghost else 0
            st.hhi[h] = max(own_and_ghost) if own_and_ghost else 0
            st.hcount[h] = int(rng.integers(0, 5))
            st.tl[h, :len(raw)] = raw[:HT_CAP]
            st.tl[h, len(raw):] = rng.integers(0, T, HT_CAP - min(len(raw), HT_CAP))          # (valid tiles, but behind the list: not to be read)
            st.tcnt[h] = HT_CAP + 1 if sp.get("overflow") else len(raw)
            if sp.get("overflow"):
                cl.add("tcnt = HT_CAP + 1 (window scan over hlo..hhi)")
        c = Case(name, cl, state=st)
        new = ref_centroid(st)
        for h in range(1, S0 + 1):
            n = int(new.hcount[h])
            if n in (0, 63, 64, 65):
                c.classes.add("%d leaves" % n)
            r = int(st.tcnt[h]) + (1 if st.ghost_active[h] and not st.ghost_done[h] else 0)
            if r in (15, 16, 17):
                c.classes.add("list of %d raw entries" % r)
            if st.tcnt[h] <= HT_CAP and new.tcnt[h] < len(set(st.tl[h, :st.tcnt[h]].tolist())):
                c.classes.add("stale tiles in a list")
        c.classes.add("S0 = %d" % S0 if S0 < 10 else "S0 of a few hundred" if S0 >= 200 else "S0 = %d" % S0)
        c.classes.add("gx = 1" if (gx == 1 or (gx == 0 and S0 <= 4)) else "gx of several")
        out.append(c)

    few = lambda n, **kw: [dict(tiles=1, leaves=int(rng.integers(1, 12)), **kw) for _ in range(n)]
    for S0 in (1, 3, 4, 5):
        build("S0 = %d" % S0, [], S0, 48 * S0, few(S0))
        build("S0 = %d, a ghost each" % S0, [], S0, 40 * S0 + 3, few(S0, ghost="active"))
    big = 300
    specs = []
    for raw in (14, 15, 16, 17):
        specs += [dict(tiles=6, leaves=30, stale=3, raw=raw), dict(tiles=6, leaves=30, stale=2, raw=raw, ghost="active"), dict(tiles=raw, leaves=40, raw=raw)]
    for n in (63, 64, 65, 100):
        specs += [dict(tiles=2, leaves=n), dict(tiles=5, leaves=n, stale=2), dict(tiles=9, leaves=n, ghost="active"), dict(tiles=1 if n <= 64 else 2, leaves=n, ghost="own")]
    specs += [dict(tiles=0, leaves=0), dict(tiles=1, leaves=0), dict(tiles=0, leaves=0, stale=3), dict(tiles=0, leaves=0, ghost="done"), dict(tiles=0, leaves=0, ghost="inactive")]
    specs += [dict(tiles=3, leaves=20, overflow=True), dict(tiles=7, leaves=70, overflow=True, ghost="active"), dict(tiles=2, leaves=5, ghost="done"), dict(tiles=2, leaves=5, ghost="inactive"),
              dict(tiles=20, leaves=50, raw=40), dict(tiles=30, leaves=64, raw=70, stale=10), dict(tiles=4, leaves=9, ghost="active"), dict(tiles=0, leaves=0, ghost="active")]
    while len(specs) < big:
        specs.append(dict(tiles=int(rng.integers(1, 9)), leaves=int(rng.integers(1, 60)), stale=int(rng.integers(0, 3)), raw=int(rng.integers(0, 14)),
                          ghost=rng.choice([None, None, None, "active", "done", "own"])))
    order = rng.permutation(big)
    specs = [specs[i] for i in order]
    build("300 helpers", ["both paths"], big, 48 * big - 5, specs)
    build("300 helpers, one workgroup", ["both paths"], big, 48 * big, [specs[i] for i in rng.permutation(big)], gx=1)
    build("301 helpers, 7 workgroups", ["both paths"], 301, 47 * 301, [specs[i] for i in rng.permutation(big)] + [dict(tiles=2, leaves=64)], gx=7)
    build("1203 helpers", ["both paths"], 1203, 40 * 1203, [dict(tiles=int(rng.integers(1, 6)), leaves=int(rng.integers(0, 50)), stale=int(rng.integers(0, 2)),
                                                             ghost=rng.choice([None, None, "active"])) for _ in range(1203)])
    return out


REQUIRED["centroid"] = (["list of %d raw entries" % n for n in (15, 16, 17)] + ["stale tiles in a list", "63 leaves", "64 leaves", "65 leaves", "0 leaves",
                        "tcnt = HT_CAP + 1 (window scan over hlo..hhi)", "ghost done", "ghost active", "S0 = 1", "S0 = 3", "S0 = 4", "S0 = 5", "S0 of a few hundred", "gx = 1", "gx of several"])


def helper_leaves(st, h):
    """(leaves in ascending ordinal, tiles holding an owned leaf ascending, ghost still active) as d_centroid sees helper h"""
    gact = bool(st.ghost_active[h]) and not st.ghost_done[h]
    gv = int(st.ghost_vox[h]) if gact else -1
    tiles = ref_tile_list(st.tl[h], int(st.tcnt[h]), gv)
    if tiles is None:
        b = int(st.hlo[h]) >> 6
        tiles = list(range(b, (int(st.hhi[h]) >> 6) + 1))
    leaves, kept = [], []
    for t in tiles:
        v = np.arange(t * 64, min(t * 64 + 64, st.V))
        own = st.owner[v] == h
        if own.any():
            kept.append(t)
        leaves += v[own | (v == gv)].tolist()
    return leaves, kept, gact


def centroid_finish(s, count):
    """a_centroid_finish (csrc/f3ds_algo.h) step by step in float32"""
    row = np.zeros(12, F)
    nx, ny, nz = s[6], s[7], s[8]
    z = F(F(F(nx * nx) + F(ny * ny)) + F(F(nz * nz) + F(0.0)))
    if z > 0:
        q = np.sqrt(z, dtype=F)
        nx, ny, nz = F(nx / q), F(ny / q), F(nz / q)
    cf = F(count)
    for k in range(6):
        row[k] = F(s[k] / cf)
    row[6], row[7], row[8] = nx, ny, nz
    return row


def ref_centroid(st):
    """the state d_centroid leaves at sweep 0 (every helper 1..S0 is recomputed)"""
    new = st.copy()
    with np.errstate(all="ignore"):
        for h in range(1, st.S0 + 1):
            leaves, kept, gact = helper_leaves(st, h)
            new.ghost_active[h] = 1 if gact else 0
            new.ghost_done[h] = 0
            new.hcount[h] = len(leaves)
            new.tcnt[h] = len(kept) if len(kept) <= HT_CAP else HT_CAP + 1
            new.tl[h, :min(len(kept), HT_CAP)] = kept[:HT_CAP]
            if leaves:
                s = np.zeros(9, F)
                for v in leaves:
                    s = (s + st.vf[v, 0:9]).astype(F)          # float32, one leaf after the other
                new.hc[h] = centroid_finish(s, len(leaves))
    return new


def slow_centroid_sums(st, h):
    """the nine sums of helper h, element by element"""
    leaves = helper_leaves(st, h)[0]
    s = [F(0)] * 9
    for v in leaves:
        for k in range(9):
            s[k] = F(s[k] + st.vf[v, k])
    return np.array(s, F), len(leaves)


# ---- d_sv_fill --------------------------------------------------------------------------------------------------------------------------------
REQUIRED["sv_fill"] = ["len == 0 helpers", "S0 not a multiple of 4", "helpers of more than 64 leaves", "helpers with a ghost leaf", "S0 of a few hundred"]


def sv_fill_states():
    """the states d_centroid leaves on centroid_states() (its reference: the GPU test of d_centroid holds the device to it)"""
    out = []
    for c in centroid_states():
        st = ref_centroid(c.state)
        cl = set()
        if (st.hcount[1:] == 0).any():
            cl.add("len == 0 helpers")
        if st.S0 % 4:
            cl.add("S0 not a multiple of 4")
        if (st.hcount > 64).any():
            cl.add("helpers of more than 64 leaves")
        if st.ghost_active.any():
            cl.add("helpers with a ghost leaf")
        if st.S0 >= 200:
            cl.add("S0 of a few hundred")
        out.append(Case(c.name, cl, state=st))
    return out


def sv_garbage(S0):
    """what racc0 / rrec0 hold before the kernel: the host layer does not clear them"""
    return np.full((S0 + 1, 12), 0x7FC12345, U32).view(F), np.full((S0 + 1, 16), 0x7FC54321, U32).view(F)


def ref_sv_fill(st, host_sv):
    """host_sv(vf, leaves) -> (rows[n x 12], acc[12], lab[3]): a_payload_row / a_fold_row / n_rgb2lab from the g++ build of the shared header.
    Returns loff, rows, row_voxel, racc0, rcnt0, rrec0, ralive0, n_alive"""
    S0, V = st.S0, st.V
    loff = np.r_[0, np.cumsum(st.hcount)].astype(U32)
    rows = np.zeros((V + S0 + 1, 12), F); row_voxel = np.zeros(V + S0 + 1, np.int32)
    racc0, rrec0 = sv_garbage(S0)
    rcnt0 = np.zeros(S0 + 1, U32); ralive0 = np.zeros(S0 + 1, np.uint8)
    alive = 0
    for h in range(1, S0 + 1):
        leaves = helper_leaves(st, h)[0]
        assert len(leaves) == st.hcount[h], (h, len(leaves), st.hcount[h])
        if not leaves:
            racc0[h] = 0; rrec0[h] = 0
            continue
        r, acc, lab = host_sv(st.vf, leaves)
        o = int(loff[h])
        rows[o:o + len(leaves)] = r; row_voxel[o:o + len(leaves)] = leaves
        racc0[h] = acc; rcnt0[h] = len(leaves); ralive0[h] = 1; alive += 1
        rrec0[h] = np.r_[st.hc[h, 0:3], st.hc[h, 6:9], acc[9:12], lab, np.zeros(4, F)].astype(F)
    return loff, rows, row_voxel, racc0, rcnt0, rrec0, ralive0, alive


def slow_sv(vf, leaves):
    """a_payload_row / a_fold_row in numpy float32, element by element (the colour truncation as C casts it: values in [0, 2^32))"""
    rows = np.zeros((len(leaves), 12), F); acc = np.zeros(12, F)
    for j, v in enumerate(leaves):
        x, y, z = vf[v, 0], vf[v, 1], vf[v, 2]
        rows[j, :9] = [F(x * x), F(x * y), F(x * z), F(y * y), F(y * z), F(z * z), x, y, z]
        rows[j, 9:] = [F(int(vf[v, k]) & 255) for k in (3, 4, 5)]
        for k in range(9):
            acc[k] = F(acc[k] + rows[j, k])
        inv = F(F(1) / F(j + 1))
        for k in range(9, 12):
            acc[k] = F(acc[k] + F(inv * F(rows[j, k] - acc[k])))
    return rows, acc


# ---- the seed stage: d_chunkbox + d_seed_grow, d_seed_nn, d_seed_filter on hand-built tables ------------------------------------------------------
# The positions are those of the lattice cases of seed_clouds_common.py (voxel_res = 2^-6: ties and bounds are hit exactly), taken as voxel centroids directly, in the
# order the case lists them: no voxelisation, no leaf order, no sort in front of the kernel under test.  The references are seed_clouds_common.reference() restricted to
# the tables; slow_*: the literal point-by-point growth loop, and the search over the 27 cells around a cell (what the oracle does) against the search over all voxels.
import seed_clouds_common as S  # noqa: E402

MAX_SEED_EVENTS = S.MAX_SEED_EVENTS
REQUIRED["seed_grow"] = ["A%d" % i for i in range(1, 8)] + ["random"]
REQUIRED["seed_nn"] = ["B%d" % i for i in range(1, 7)] + ["D: large offsets", "D: offset 0", "in-lane ties", "in-lane ties, higher ordinal first"]
REQUIRED["seed_filter"] = ["C%d" % i for i in range(1, 6)] + ["pruning margin", "min_points an integer"]


def _voxels_of(name, reverse=False, shuffle=None):
    """The distinct points of a case's frame, in frame order (reverse: last first; shuffle: the first stays -- the grid starts from it --, the others in an order drawn from that seed)."""
    xyz = S.frame_of(name)[:, :3]
    _, first = np.unique(xyz, axis=0, return_index=True)
    xyz = xyz[np.sort(first)]
    if shuffle is not None:
        xyz = np.vstack([xyz[:1], xyz[1:][np.random.default_rng(shuffle).permutation(len(xyz) - 1)]])
    return np.ascontiguousarray(xyz[::-1] if reverse else xyz, F)


def vf_rows(xyz):
    vf = np.zeros((len(xyz), 12), F)
    vf[:, :3] = xyz
    return vf


def seed_grow_cases():
    prm = lambda n: S.CASE[n].params["seed_res"]
    out = [Case(n, cls, xyz=_voxels_of(n), seed_res=prm(n), cond=S.CASE[n].cond) for cls, n in (
        ("A2", "a2-triggers-at-0-255-256"), ("A3", "a3-two-events-in-a-chunk"), ("A4", "a4-event-at-the-last-voxel"), ("A6", "a6-thirteen-events"),
        ("A7", "a7-cube-edge"))]
    # A5: the first voxel in the middle, the others below and above it on every axis (positions in voxels of 2^-6, seed_res two of them)
    a5 = np.array([(10.5, 10.5, 10.5), (0.25, 0.25, 20.5), (20.5, 20.5, 0.25), (23.75, 20.5, 20.5), (20.5, 23.75, 20.5), (20.5, 20.5, 23.75)], F) * F(S.RD)
    a1 = np.array([(0, 0, 0), (1, 0, 0), (0, 2, 1), (3, 3, 3), (7.5, 7.5, 7.5)], F) * F(S.RD)
    out.append(Case("a1-single-cell", "A1", xyz=a1, seed_res=8 * S.RD, cond=("events", 1, 1)))
    out.append(Case("a5-every-direction", "A5", xyz=a5, seed_res=2 * S.RD, cond=("directions",)))
    rng = np.random.default_rng(77)
    for i in range(30):
        n = int(rng.integers(1, 3000))
        spread = float(rng.choice([0.5, 4.0, 40.0, 600.0]))
        xyz = (rng.normal(0.0, spread, (n, 3)) + rng.uniform(-100, 100, 3)).astype(F)
        out.append(Case("random %d" % i, "random", xyz=xyz, seed_res=float(F(rng.choice([0.02, 0.08, 0.5]))), cond=None))
    return out


def ref_seed_grow(c):
    return S.grow_grid(c.xyz, c.seed_res)


def slow_seed_grow(c):
    """adoptBoundingBoxToPoint point by point: (final minimum, depth, keys, [(trigger, depth)])."""
    res = float(F(c.seed_res)); eps = S.FLT_EPS
    mn = [0.0] * 3; mx = [0.0] * 3
    depth, defined, keys, ev = 0, False, [], []
    for i, p in enumerate(np.asarray(c.xyz, np.float64).tolist()):
        while True:
            up = [p[a] >= mx[a] for a in range(3)]
            if defined and not any(up) and not any(p[a] < mn[a] for a in range(3)):
                break
            if defined:
                side = float(1 << depth) * res
                for a in range(3):
                    if not up[a]:
                        mn[a] -= side
                        for k in keys:
                            k[a] += 1 << depth
                depth += 1
                mx = [mn[a] + (float(1 << depth) * res - eps) for a in range(3)]
            else:
                mn = [p[a] - res - 0.0 for a in range(3)]       # (the cube of two cells a side around the first point: min = p - res / 2 - res / 2)
                mn = [(p[a] - res / 2) - (2.0 * res - ((p[a] + res / 2) - (p[a] - res / 2))) / 2.0 for a in range(3)]
                mx = [(p[a] + res / 2) + (2.0 * res - ((p[a] + res / 2) - (p[a] - res / 2))) / 2.0 for a in range(3)]
                depth, defined = 1, True
            ev.append((i, depth))
        keys.append([int((p[a] - mn[a]) / res) for a in range(3)])
    return mn, depth, np.array(keys, np.int64), ev


class SeedTable:
    """The arrays seg_seeds hands to d_seed_nn / d_seed_filter for voxel centroids xyz: the cell keys, the voxels sorted by cell (Morton order of the cells, ordinals
    ascending inside a cell, as the stable radix sort leaves them), the cell starts, the grid."""

    def __init__(self, xyz, seed_res, voxel_res, descending=False):
        self.xyz = np.ascontiguousarray(xyz, F)
        self.seed_res, self.voxel_res = seed_res, voxel_res
        self.ref = S.reference(self.xyz, seed_res, voxel_res)
        g = self.ref.grid
        self.V = len(self.xyz)
        self.vf = vf_rows(self.xyz)
        self.ckey = np.ascontiguousarray(g.keys, U32)
        self.sorted_vox = np.ascontiguousarray(np.argsort(self.ref.cell_of, kind="stable"), U32)
        self.C = len(self.ref.cell_keys)
        self.cell_start = np.zeros(self.C + 1, U32)
        self.cell_start[1:] = np.cumsum(np.bincount(self.ref.cell_of, minlength=self.C))
        if descending:      # a cell's list with the highest ordinal first: the kernels' minimum under (distance, ordinal) does not depend on the order they visit a list in
            for c in range(self.C):
                self.sorted_vox[self.cell_start[c]:self.cell_start[c + 1]] = self.sorted_vox[self.cell_start[c]:self.cell_start[c + 1]][::-1].copy()
        self.grid = np.array([g.res, g.min[0], g.min[1], g.min[2]], np.float64)
        self.r2 = S.radius_sq(seed_res)
        self.min_points = S.min_points(seed_res, voxel_res)


def _table_case(cls, name, reverse=False, shuffle=None):
    p = S.CASE[name].params
    return Case(name, cls, table=SeedTable(_voxels_of(name, reverse, shuffle), p["seed_res"], p["voxel_res"]), cond=S.CASE[name].cond)


TIE_AT = (5, 69, 100, 261)      # list positions of the four tied voxels: 5, 69 and 261 fall to lane 5 (the second of its four entries of a round, and the next round)


def _tie_table(descending):
    """One cell of 304 voxels: four at distance 1 from its centre, at the list positions TIE_AT, 300 further out.  With the list descending the lane that holds three
    of the tied voxels meets the highest ordinal first and the lowest -- the answer -- last."""
    m = S.M
    centre = (np.array([2, 2, 2]) + 0.5) * m
    fill = S.cell_slots(m, (2, 2, 2))
    fill = fill[((fill - centre) ** 2).sum(axis=1) >= 4.0][:300]
    tied = [centre + (1, 0, 0), centre - (1, 0, 0), centre + (0, 1, 0), centre - (0, 1, 0)]
    cell, k = [], 0
    for pos in range(304):
        if pos in TIE_AT:
            cell.append(tied[TIE_AT.index(pos)])
        else:
            cell.append(fill[k]); k += 1
    cell = np.array(cell)
    q = np.vstack([[[0, 0, 0]], cell[::-1] if descending else cell])      # (voxel 0 starts the grid; descending: the list's first entry is the last voxel)
    return SeedTable((q * S.RD).astype(F), m * S.RD, S.RD, descending=descending)


def seed_nn_cases():
    return [Case("ties 64 and 256 entries apart, list ascending", "in-lane ties", table=_tie_table(False), cond=None),
            Case("ties 64 and 256 entries apart, list descending", ["in-lane ties", "in-lane ties, higher ordinal first"], table=_tie_table(True), cond=None),
            _table_case("B1", "b1-shortcut-and-not"), _table_case(["B2", "B7"], "b2-b7-corner-cut"), _table_case("B3", "b3-ties", shuffle=3), _table_case("B4", "b4-key-zero", reverse=True),
            _table_case("B5", "b5-cell-sizes"), _table_case("B6", "b6-big-blocks"), _table_case("D: large offsets", "d-offset-600"), _table_case("D: offset 0", "d-offset-0")]


def seed_filter_cases():
    return [_table_case("C1", "c1-counts"), _table_case("C2", "c2-at-the-radius"), _table_case("C3", "c3-eight-cells"), _table_case("C4", "c4-own-cell-only"),
            _table_case("C5", "c5-pruned-neighbours"), _table_case("pruning margin", "c8-face-near-the-radius"), _table_case("min_points an integer", "c9-min-points-exactly-2"),
            _table_case("B6 totals", "b6-big-blocks"), _table_case("B5 totals", "b5-cell-sizes")]


def ref_seed_nn(t):
    return t.ref.seed_orig


def ref_seed_filter(t):
    return t.ref.keep.astype(U32)


def _block27(t, key):
    by_key = {tuple(k): c for c, k in enumerate(t.ref.cell_keys.tolist())}
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                c = by_key.get((key[0] + dx, key[1] + dy, key[2] + dz))
                if c is not None:
                    out.append(np.nonzero(t.ref.cell_of == c)[0])
    return np.sort(np.concatenate(out))


def slow_seed_nn(t):
    """The nearest voxel among the 27 cells around each cell only (the oracle's search)."""
    out = np.zeros(t.C, np.int32)
    for c, key in enumerate(t.ref.cell_keys.tolist()):
        cand = _block27(t, key)
        d = S.sqdist(t.ref.centres[c], t.xyz[cand])
        out[c] = cand[int(np.argmin(d))]
    return out


def slow_seed_filter(t, seed_orig):
    out = np.zeros(t.C, U32)
    for c, s in enumerate(seed_orig):
        cand = _block27(t, t.ref.grid.keys[s].tolist())
        out[c] = int((S.sqdist(t.xyz[s], t.xyz[cand]) < t.r2).sum()) > t.min_points
    return out
