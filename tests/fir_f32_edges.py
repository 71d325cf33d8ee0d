"""arm_fir_f32 stage (msdr_fir_f32_process): the census of level steps, spikes and range edges, and the judge that holds every kernel
of the stage to the precision clause of include/msdr.h (msdr_fir_f32_set_input_range).  numpy only: tests/test_fir_f32_edges.py runs
the judge on the CPU (an emulation of the split-fp16 arithmetic, three mutants of it, the sequential fp32 oracle),
tests/test_gpu_fir_f32_edges.py and tests/debug/fuzz_fir_f32.py run it on the library's outputs.

Positions are relative to a call: the kernels restart their 1024-output tiles at every call, and the numTaps - 1 samples before a call
are the carried history.  The functions window_lo / pinned_mw below ARE the header's definition of a tile's scale window, per kernel;
nothing else in the judge knows about kernels."""
import numpy as np

TILE = 1024
CHANNELS = 6
LAYOUTS = {"aligned": (5 * 1024, 3 * 1024 + 332),           # every row 16-byte aligned
           "odd": (4 * 1024 + 1, 4 * 1024 + 331)}           # odd rows unaligned: their tiles take the bounds-checked path
# (numTaps, every channel taps of its own, kind, what FirF32.kernel_name() must report)
TAP_CONFIGS = [(8, False, "plain", "fir_kernel<FirF32>"), (600, False, "plain", "fir_kernel<FirF32>"),
               (16, False, "tq", "fir_f32tq_kernel<"), (100, False, "tq", "fir_f32tq_kernel<"), (256, False, "tq", "fir_f32tq_kernel<"),
               (289, False, "tq", "fir_f32tq_kernel<"),
               (290, False, "mf", "fir_f32mf_kernel"), (321, False, "mf", "fir_f32mf_kernel"), (512, False, "mf", "fir_f32mf_kernel"),
               (513, False, "mf", "fir_f32mf_kernel"),
               (100, True, "plain", "chain_f32pc_kernel"), (512, True, "plain", "chain_f32pc_kernel")]
BASES = (0, -60, 90)            # log2 of the base level; every level stays inside the header's range 2^-86 .. 2^115
SPIKE = 20                      # an isolated sample 2^20 times its row's level
STRETCH_MIN, STRETCH_HEADROOM, STRETCH_TOL = 64, 10, 1e-6


def fm_halo(ntaps):
    return ((ntaps - 1 + 31) // 32) * 32


def kernel_name_ok(expect, name):
    return name == expect if expect in ("fir_kernel<FirF32>", "fir_f32mf_kernel") else name.startswith(expect)


# ------------------------------------------------------------------------------------------------------------------------------
# the header's scale window (msdr.h, msdr_fir_f32_set_input_range)
# ------------------------------------------------------------------------------------------------------------------------------
def window_lo(kind, ntaps, tile):
    """First sample (relative to the call; negative = carried history) of the window that sets the scale of tile `tile`:
    16 .. 289 taps ("tq"): the tile's 1024 samples and the numTaps - 1 before them rounded up to a multiple of 32;
    290 .. 513 taps ("mf"): the tile's 1024 samples and the whole tile before it.  The history holds numTaps - 1 samples."""
    back = {"tq": fm_halo(ntaps), "mf": TILE}[kind]
    return max(tile * TILE - back, -(ntaps - 1))


def pinned_mw(max_abs):
    """msdr_fir_f32_set_input_range(max_abs): one scale, Mw = max_abs rounded up to a power of two for every tile."""
    return float(2.0 ** np.ceil(np.log2(max_abs)))


# ------------------------------------------------------------------------------------------------------------------------------
# the census
# ------------------------------------------------------------------------------------------------------------------------------
def _profiles(n0, ntaps):
    """name -> (list of (position, log2 level from there on), list of spike positions); positions in the first call."""
    late = n0 - max(1, (ntaps - 1) // 2)            # inside the last numTaps - 1 samples of the first call
    return {
        "flat": ([], []),
        "drop12@tile": ([(1024, -12)], []), "drop20@tile": ([(1024, -20)], []), "drop20@+500": ([(1524, -20)], []),
        "drop20@history": ([(late, -20)], []), "drop34@tile": ([(1024, -34)], []),
        "rise20@tile": ([(2048, 20)], []), "rise20@+500": ([(2548, 20)], []), "rise30@tile": ([(2048, 30)], []),
        "rise30@+500": ([(2548, 30)], []), "loud_tile": ([(1024, 20), (2048, 0)], []),
        "spike@first": ([], [2048]), "spike@last": ([], [3071]), "spike@500": ([], [2548]),
        "drop20@segment": ([(3072, -20)], []), "rise20@segment": ([(3072, 20)], []),      # the tile that opens fir_f32mf_kernel's second segment
    }


GROUPS = {"drops": ("drop12@tile", "drop20@tile", "drop20@+500", "drop20@history", "drop34@tile"),
          "rises": ("rise20@tile", "rise20@+500", "rise30@tile", "rise30@+500", "loud_tile"),
          "spikes": ("spike@first", "spike@last", "spike@500", "drop20@segment", "rise20@segment")}
ALL_GROUPS = dict(GROUPS, flat=("flat",) * 5)                   # (not in the census: the carrier of the non-finite and out-of-range cases)
PINNED_RANGE = 8.0              # above every sample of the "drops" group at base level 1


class Spec:
    """One census case: a tap configuration, a call layout, a group of five level profiles (rows 1 .. 5; row 0 is flat), a base level."""

    def __init__(self, ntaps, per_channel, kind, kernel, layout, group, base, pinned=None):
        self.ntaps, self.per_channel, self.kind, self.kernel = ntaps, per_channel, kind, kernel
        self.layout, self.sizes, self.group, self.base, self.pinned = layout, LAYOUTS[layout], group, base, pinned
        self.rows = ("flat",) + ALL_GROUPS[group]
        self.id = "%d%s-%s-%s-%s" % (ntaps, "pc" if per_channel else "", layout, group, "pinned" if pinned else "2^%d" % base)

    def __repr__(self):
        return self.id


def census():
    specs = []
    for ntaps, pc, kind, kernel in TAP_CONFIGS:
        for layout in LAYOUTS:
            for group in GROUPS:
                for base in BASES:
                    specs.append(Spec(ntaps, pc, kind, kernel, layout, group, base))
            specs.append(Spec(ntaps, pc, kind, kernel, layout, "drops", 0, pinned=PINNED_RANGE))
    return specs


class Case:
    """The arrays of a Spec: taps [6][numTaps] (CMSIS order), samples x [6][n0 + n1] float32, log2 level per sample, steps per row."""


def build(spec):
    seed = [spec.ntaps, int(spec.per_channel), list(LAYOUTS).index(spec.layout), list(ALL_GROUPS).index(spec.group), spec.base + 100]
    rng = np.random.default_rng(seed)
    c = Case()
    c.spec = spec
    n0, n1 = spec.sizes
    n = n0 + n1
    N = spec.ntaps
    win = np.hanning(N + 2)[1:-1] + 0.05
    rows = CHANNELS if spec.per_channel else 1
    taps = (rng.standard_normal((rows, N)) * win * (1.0 + 0.5 * np.arange(N) / N)).astype(np.float32)      # asymmetric
    c.taps = np.ascontiguousarray(np.broadcast_to(taps, (CHANNELS, N)) if rows == 1 else taps)
    prof = _profiles(n0, N)
    noise = rng.standard_normal((CHANNELS, n)).astype(np.float32)
    c.lev = np.zeros((CHANNELS, n), np.int64)
    c.steps, c.spikes = [], []
    for r, name in enumerate(spec.rows):
        steps, spikes = prof[name]
        rel = np.zeros(n, np.int64)
        for pos, e in steps:
            rel[pos:] = e
        # base 2^90 is the profile's loudest level, base 2^-60 its quietest, base 1 the level it starts at
        shift = spec.base - (rel.max() if spec.base > 0 else rel.min() if spec.base < 0 else 0)
        c.lev[r] = rel + shift
        prev = [0] + [e for _, e in steps]
        c.steps.append([(pos, "drop" if e < p else "rise") for (pos, e), p in zip(steps, prev)])
        c.spikes.append(list(spikes))
    c.x = (noise * np.exp2(c.lev.astype(np.float64))).astype(np.float32)         # exact: a power of two
    for r, spikes in enumerate(c.spikes):
        for p in spikes:
            c.x[r, p] = np.float32(2.0 ** (int(c.lev[r, p]) + SPIKE))
    assert np.isfinite(c.x).all() and float(np.abs(c.x).max()) < 2.0 ** 115 and float(np.abs(c.x[c.x != 0]).min()) > 2.0 ** -110
    if spec.pinned:
        assert float(np.abs(c.x).max()) < spec.pinned
    return c


def calls(case):
    """(call index, first sample, length, history [6][numTaps - 1]) of every call of the case's layout."""
    N, o, out = case.spec.ntaps, 0, []
    for ci, m in enumerate(case.spec.sizes):
        hist = np.zeros((CHANNELS, N - 1), np.float32)
        have = min(o, N - 1)
        if have:
            hist[:, N - 1 - have:] = case.x[:, o - have:o]
        out.append((ci, o, m, hist))
        o += m
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------------------------------------
def _corr(xe, w, n):
    """sum_k w[k] xe[t + k], t = 0 .. n - 1 (float64, evaluated term by term: an FFT would smear a loud stretch's rounding over a quiet one)."""
    return np.convolve(xe, w[::-1])[w.size - 1:w.size - 1 + n]


class RowRef:
    """Truth, clause (a)'s bound and clause (b)'s stretches for one row of one call."""


def row_reference(kind, h, hist, x, lev, pinned=None):
    """Every sample of an output's window is held to max(2^-21 |x|, 2^-39 Mw), the numTaps - 1 before the tile included: on that one
    point the judge asks more than the header, whose parenthetical allows fir_f32mf_kernel 2^-27 Mw / 2^-37 Mw for a halo sample carried
    through a small change of scale."""
    N, n = h.size, x.size
    r = RowRef()
    r.kind, r.ntaps, r.n = kind, N, n
    h64 = h.astype(np.float64)
    xe = np.concatenate([hist, x]).astype(np.float64)          # xe[N - 1 + t] = sample t of the call
    ax, ah = np.abs(xe), np.abs(h64)
    r.truth = _corr(xe, h64, n)
    ntiles = (n + TILE - 1) // TILE
    if kind == "plain":
        # plain fp32 FMAs: the any-order forward bound of a numTaps-term sum, unit roundoff taken one bit wide
        r.bound = _corr(ax, 3.0 * N * 2.0 ** -23 * ah, n)
        wmax = np.lib.stride_tricks.sliding_window_view(ax, N).max(axis=1)[:n]      # an output's window: its own numTaps samples
    else:
        H = fm_halo(N)
        etap = np.maximum(2.0 ** -21 * ah, 2.0 ** -38 * ah.max())
        r.bound = _corr(ax, etap + 3.0 * (H + 32) * 2.0 ** -23 * ah, n)
        wmax = np.empty(n)
        r.mw = np.empty(ntiles)
        for i in range(ntiles):
            t0, t1 = i * TILE, min((i + 1) * TILE, n)
            lo = window_lo(kind, N, i)
            mw = pinned_mw(pinned) if pinned else float(ax[N - 1 + lo:N - 1 + t1].max())
            r.mw[i] = mw
            wmax[t0:t1] = mw
            ex = np.maximum(2.0 ** -21 * ax[N - 1 + t0 - (N - 1):N - 1 + t1], 2.0 ** -39 * mw)
            r.bound[t0:t1] += _corr(ex, ah, t1 - t0)
    # clause (b): maximal runs of >= 64 outputs of one level whose window holds nothing above 2^10 times that level
    r.stretches = []
    if not pinned:                                              # a pinned scale makes the absolute bound only
        ok = wmax <= np.exp2(lev.astype(np.float64) + STRETCH_HEADROOM)
        cuts = np.flatnonzero((ok[1:] != ok[:-1]) | (lev[1:] != lev[:-1])) + 1
        for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n]])):
            if ok[a] and b - a >= STRETCH_MIN:
                r.stretches.append((int(a), int(b)))
    r.covered = sum(b - a for a, b in r.stretches) / float(n)
    return r


def judge_row(ref, got, exclude=None):
    """-> (mask of outputs that miss clause (a), list of (lo, hi, relative RMS) of stretches that miss clause (b), the largest
    error / bound over the judged outputs that are finite: above 1 where one misses).
    exclude: outputs that are not judged at all (the tile windows of a non-finite sample)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref.truth)
    bad = ~(err <= ref.bound)                                   # (a NaN or an output never written misses)
    judged = np.isfinite(err) & (err > 0)
    if exclude is not None:
        bad &= ~exclude
        judged &= ~exclude
    with np.errstate(divide="ignore"):
        worst = float((err[judged] / ref.bound[judged]).max()) if judged.any() else 0.0
    missed = []
    for a, b in ref.stretches:
        if exclude is not None and exclude[a:b].any():
            continue                                            # (held by clause (a) where it is judged)
        d, t = got[a:b] - ref.truth[a:b], ref.truth[a:b]
        rms = float(np.sqrt((d * d).sum() / max((t * t).sum(), 1e-300)))
        if not rms < STRETCH_TOL:
            missed.append((a, b, rms))
    return bad, missed, worst


def far_edge(kind, ntaps, sizes, pos, what):
    """Where clause (b) must pick up again behind a step at `pos` (absolute sample): at a rise, the step itself (the loud outputs are the
    level of their window); at a drop, the first tile (of >= 64 outputs) whose window is free of loud samples -- for the plain-fp32 kernels
    the first output whose numTaps samples are."""
    if what == "rise":
        return pos
    if kind == "plain":
        return pos + ntaps - 1
    o = 0
    for m in sizes:
        for i in range((m + TILE - 1) // TILE):
            if o + window_lo(kind, ntaps, i) >= pos and min(TILE, m - i * TILE) >= STRETCH_MIN:
                return o + i * TILE
        o += m
    return None


def case_references(case):
    """[call][row] -> RowRef."""
    s = case.spec
    return [[row_reference(s.kind, case.taps[r], hist[r], case.x[r, o:o + m], case.lev[r, o:o + m], pinned=s.pinned)
             for r in range(CHANNELS)] for _, o, m, hist in calls(case)]


def strike(case, struck):
    """Samples a caller may not expect precision around (non-finite, or outside the magnitude range): struck = {row: {position: value}}.
    -> (the case as the library sees it, the clean case the judge takes its truth from -- the struck samples zero --, exclude[call][row]:
    the outputs whose tile window holds a struck sample, or whose history still does.  Every other output is judged in full: the struck
    sample is outside its window, so it must not have met it)."""
    s = case.spec
    dirty, clean = Case(), Case()
    for c in (dirty, clean):
        c.__dict__.update(case.__dict__)
        c.x = case.x.copy()
    exclude = [[None] * CHANNELS for _ in s.sizes]
    for r, hits in struck.items():
        for p, v in hits.items():
            dirty.x[r, p], clean.x[r, p] = v, 0.0
        for ci, o, m, _ in calls(case):
            mask = np.zeros(m, bool)
            for p in hits:
                q = p - o                                       # relative to the call
                if s.kind == "plain":                           # the numTaps outputs that read the sample
                    mask[max(0, q):max(0, min(m, q + s.ntaps))] = True
                    continue
                for i in range((m + TILE - 1) // TILE):         # the tiles whose scale window holds it
                    t1 = min((i + 1) * TILE, m)
                    if window_lo(s.kind, s.ntaps, i) <= q < t1:
                        mask[i * TILE:t1] = True
            exclude[ci][r] = mask
    return dirty, clean, exclude


def coverage_gaps(case, refs):
    """Steps behind which no clause (b) stretch starts within numTaps outputs of the far edge: must be empty."""
    s, gaps = case.spec, []
    if s.pinned:
        return gaps
    starts = [[o + a for (_, o, _, _), row in zip(calls(case), refs) for a, _ in row[r].stretches] for r in range(CHANNELS)]
    for r in range(CHANNELS):
        for pos, what in case.steps[r]:
            e = far_edge(s.kind, s.ntaps, s.sizes, pos, what)
            if e is None or not any(pos <= a <= e + s.ntaps for a in starts[r]):      # (a few small loud samples may let it start early)
                gaps.append((s.rows[r], pos, what, e))
    return gaps


def judge_case(case, refs, outputs, exclude=None):
    """outputs[call] = [6][m] -> list of violation records (empty = the case passes); exclude[call][row] = mask or None."""
    s, out = case.spec, []
    for (ci, o, m, _), row in zip(calls(case), refs):
        for r in range(CHANNELS):
            ex = exclude[ci][r] if exclude is not None else None
            bad, missed, worst = judge_row(row[r], outputs[ci][r], ex)
            if bad.any():
                for i in range((m + TILE - 1) // TILE):
                    t0, t1 = i * TILE, min((i + 1) * TILE, m)
                    idx = np.flatnonzero(bad[t0:t1])
                    if idx.size:
                        g = np.asarray(outputs[ci][r], np.float64)
                        k = t0 + idx[np.nanargmax(np.where(np.isfinite(g[t0 + idx]), np.abs(g[t0 + idx] - row[r].truth[t0 + idx]) / row[r].bound[t0 + idx], np.inf))]
                        out.append(dict(clause="a", call=ci, channel=r, profile=s.rows[r], tile=i, first=int(idx[0]), last=int(idx[-1]), count=int(idx.size),
                                        nan=int(np.isnan(g[t0 + idx]).sum()), at=int(k), got=float(g[k]), want=float(row[r].truth[k]),
                                        over=float(abs(g[k] - row[r].truth[k]) / row[r].bound[k])))
            for a, b, rms in missed:
                out.append(dict(clause="b", call=ci, channel=r, profile=s.rows[r], tile=a // TILE, first=a, last=b - 1, rms=rms))
    return out


def format_violations(spec, kernel, viol, limit=40):
    """The (call, channel, tile) map of a failed case."""
    lines = ["%s  kernel %s: %d violations" % (spec.id, kernel, len(viol))]
    for v in viol[:limit]:
        if v["clause"] == "a":
            lines.append("   (a) call %d channel %d [%s] tile %d: %d outputs in +%d .. +%d (%d NaN); worst at +%d got %.9g want %.9g = %.3g x the bound" % (
                v["call"], v["channel"], v["profile"], v["tile"], v["count"], v["first"], v["last"], v["nan"], v["at"], v["got"], v["want"], v["over"]))
        else:
            lines.append("   (b) call %d channel %d [%s] stretch +%d .. +%d (from tile %d): relative RMS %.3g" % (
                v["call"], v["channel"], v["profile"], v["first"], v["last"], v["tile"], v["rms"]))
    return "\n".join(lines)
