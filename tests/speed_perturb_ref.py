"""Reference for the per-row resampler / speed perturbation, written from the header text (include/amdspeech.h, "per-row resampler /
speed perturbation"), not from the kernel (csrc/frontend.hip: resample_rows_kernel, ops.resample_rows).

Lengths and the draw are restated in Python integers; the waveform reference is the float64 oracle of the existing resampler,
oracle.frontend.resample_kaiser_best(x, rate_in * permille, rate_out * 1000) -- a signal played f times faster is the signal
resampled from rate * f to rate -- and a row with num == den is x itself.  The case table of the GPU test and the plan the header
documents live here too, so that the CPU test can hold the plan against the library without a device.
"""
import numpy as np

from oracle import frontend as ofe

TILE = 1024                     # outputs per workgroup (amdspeech_resample_rows_plan_info.tile)
TABLE_CHUNK = 4097              # table entries of a staged chunk
NWIN, TABLE = 32769, 512        # kaiser_best: 64 zero crossings * 512 entries + 1, entries per crossing
PERMILLE_MIN, PERMILLE_MAX = 500, 2000
BOUND = 2e-5                    # the bound tests/test_gpu_frontend.py holds amdspeech_resample to
DRAW_STREAM = 0x5B000000
M32 = 0xFFFFFFFF
POISON = np.float32(np.nan)


# ------------------------------------------------------------------------------------------------ lengths
def num_den(rate_in, rate_out, permille):
    return rate_out * 1000, rate_in * permille


def n_total(n, rate_in, rate_out, permille):
    """ceil(n * num / den), exact."""
    num, den = num_den(rate_in, rate_out, permille)
    return -((-n * num) // den)


def n_interp(n, rate_in, rate_out, permille):
    """(int)((double)n * ratio): the samples the interpolation produces; the rest up to n_total is padding."""
    num, den = num_den(rate_in, rate_out, permille)
    return int(float(n) * (float(num) / float(den)))


def is_copy(rate_in, rate_out, permille):
    num, den = num_den(rate_in, rate_out, permille)
    return num == den


# ------------------------------------------------------------------------------------------------ the draw
def _mix32(v):
    v &= M32
    v ^= v >> 16
    v = (v * 0x7feb352d) & M32
    v ^= v >> 15
    v = (v * 0x846ca68b) & M32
    v ^= v >> 16
    return v


def random24(seed, stream, idx):
    """SpecAugment's documented hash: mix32(mix32(idx ^ lo32(seed)) + stream * 0x9e3779b9 + hi32(seed)) >> 8."""
    a = _mix32((idx ^ (seed & M32)) & M32)
    return _mix32((a + stream * 0x9e3779b9 + (seed >> 32)) & M32) >> 8


def draw(seed, index, factors):
    idx = ((index & M32) + (index >> 32) * 0x9E3779B1) & M32
    return factors[(random24(seed & 0xFFFFFFFFFFFFFFFF, DRAW_STREAM, idx) * len(factors)) >> 24]


# ------------------------------------------------------------------------------------------------ the plan
def row_span(n, rate_in, rate_out, permille):
    num, den = num_den(rate_in, rate_out, permille)
    ratio = float(num) / float(den)
    step = int(min(1.0, ratio) * TABLE)
    return min(n, int((TILE - 1) / ratio) + 2 * (NWIN // step) + 4)


def expected_plan(n_samples, permille, rate_in, rate_out, out_max=None):
    if out_max is None:
        out_max = max([n_total(n, rate_in, rate_out, p) for n, p in zip(n_samples, permille)] + [1])
    B = len(n_samples)
    spans = [row_span(n, rate_in, rate_out, p) for n, p in zip(n_samples, permille) if n > 0 and not is_copy(rate_in, rate_out, p)]
    tiles = -(-out_max // TILE)
    span = max(spans + [0])
    chunk = TABLE_CHUNK if span else 0
    return dict(tile=TILE, tiles_per_row=tiles, workgroups=tiles * B, span_max=span, table_chunk=chunk,
                lds_bytes=-(-4 * span // 16) * 16 + 8 * chunk, any_copy=int(any(is_copy(rate_in, rate_out, p) for p in permille)), meta_launches=-(-2 * B // 512))


# ------------------------------------------------------------------------------------------------ signals and waveforms
def signal(n, rate, seed):
    """The sine-plus-noise mix of test_resampler_matches_oracle_and_scipy, amplitude below 1."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    return (0.5 * np.sin(2 * np.pi * 440 * t) + 0.3 * np.sin(2 * np.pi * 1234.5 * t + 0.7) + 0.01 * rng.randn(n)).astype(np.float32)


def reference_row(x, rate_in, rate_out, permille):
    """float64 [n_total]: the interpolated samples, then the 0 or 1 padding zeros; a copy row is x itself."""
    if is_copy(rate_in, rate_out, permille):
        return np.asarray(x, np.float64)
    y = ofe.resample_kaiser_best(x, rate_in * permille, rate_out * 1000)
    assert len(y) == n_total(len(x), rate_in, rate_out, permille), (len(y), len(x), rate_in, rate_out, permille)
    return y


SPECIALS = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000,
                     0x3F800000], np.uint32)      # -0.0, denormals, +-inf, quiet and signalling NaN payloads, 0, 1


def _special_row(n, seed):
    rng = np.random.RandomState(seed)
    return SPECIALS[rng.randint(0, len(SPECIALS), n)].view(np.float32)


def _tile_edge_lengths(rate_in, rate_out, permille, k):
    """Input lengths whose n_total is j * TILE - 1, j * TILE and j * TILE + 1, each with the first j >= k at which some length gives
    it (when up-sampling not every output length occurs)."""
    out = []
    for d in (-1, 0, 1):
        for j in range(k, k + 64):
            want = j * TILE + d
            n = want * rate_in * permille // (rate_out * 1000)
            while n_total(n, rate_in, rate_out, permille) < want:
                n += 1
            if n_total(n, rate_in, rate_out, permille) == want:
                out.append(n)
                break
    assert len(out) == 3
    return out


def cases():
    """name -> (rate_in, rate_out, [(n, permille)], special): the issue's table.  special: rows whose input is bit patterns."""
    edge = _tile_edge_lengths(16000, 22050, 1000, 2) + _tile_edge_lengths(16000, 22050, 900, 3) + _tile_edge_lengths(16000, 22050, 1100, 1)
    return {
        "edges16k": (16000, 22050, [(0, 1000), (1, 900), (2, 1100), (63, 1000), (64, 900), (129, 1100), (3000, 900), (3000, 1000),
                                    (3000, 1100)], ()),
        "down": (44100, 22050, [(63, 2000), (3000, 2000), (3000, 500), (2999, 1000), (3000, 1100)], ()),
        "up": (8000, 22050, [(2500, 500), (700, 2000)], ()),
        "identity": (22050, 22050, [(700, 1000), (1, 1000), (257, 1000), (1800, 1000), (1800, 900), (1800, 1100)], (0, 1, 2, 3)),
        "tile_edges": (16000, 22050, list(zip(edge, [1000] * 3 + [900] * 3 + [1100] * 3)), ()),
        "wide": (16000, 22050, [(40 + (37 * b) % 61, (900, 1000, 1100)[b % 3]) for b in range(513)], ()),
    }


_BUILT = {}


def built(name):
    """(rate_in, rate_out, n [B], permille [B], host [B][n_max] float32 with NaN poison at and past each row's n, refs: float64
    rows of n_total samples).  Computed once per process and shared; the callers do not modify it."""
    if name not in _BUILT:
        rate_in, rate_out, rows, special = cases()[name]
        n = [r[0] for r in rows]
        pm = [r[1] for r in rows]
        n_max = max(max(n), 1)
        host = np.full((len(rows), n_max), POISON, np.float32)
        refs = []
        for b, (k, p) in enumerate(rows):
            x = _special_row(k, 100 + b) if b in special else signal(k, rate_in, 1000 * len(name) + b)
            host[b, :k] = x
            refs.append(x.copy() if b in special else reference_row(x, rate_in, rate_out, p))
        _BUILT[name] = (rate_in, rate_out, n, pm, host, refs)
    return _BUILT[name]
