"""The cases of tests/test_gpu_bands.py, crafted and pinned on the CPU before they are used on the device.

The greedy selection scores a candidate row in a cheap tier first (csrc/select_dev.h): COARSE
(all f32) decides a row beyond thr +- (band + coarse_band(B)), FAST (f64 fma, f32 mantissa log) beyond
thr +- (band + FAST_BAND), the exact f64 tier unless the margin is inside sel_band, where the host arbiter replays the
reference.  Random streams almost never place a row within 1e-6 of the threshold, so this module BUILDS such rows: for
every case a random prefix, then near-copies of the set's lowest member whose exact score (the oracle's) sits at the
threshold plus a chosen margin, the oracle tracking the set in the case's mode (nmost or max_divergent).  The margins:

  * multiples {0.1, 0.5, 0.9, 1.1} of FAST_BAND, both signs, and of coarse_band(B) where the case's persistent
    instantiation has a COARSE tier (count rows, B a multiple of 256 and at most 4096: read off p_scan_rows);
  * the NEAR-ZERO pair: |margin| inside [8 sel_band(B, log2 B), 0.05 FAST_BAND], one of each sign -- well outside the
    arbiter's zone, well inside what an f32 tier would get wrong every other time.  These give the device tests their
    teeth: a tier that decided them itself would flip their sign about half the time;
  * for frequency rows (T = double) a candidate (1 - t) f_low + t g has a margin continuous in t, bisected against the
    oracle: the same targets, and +-0.25 / +-3 x sel_band_min(B) for the arbiter's own edge.

What is asserted here, from the oracle alone, are the conditions under which the device tests say something: every
margin where it was aimed, every near-zero margin inside its window, the oracle's decision the sign of the margin, at
least MIN_ACCEPTS accepts beyond the seeds, no two rows equal, every bin count and row width on the intended branch.

Crafting is seeded and cached per session (functools.lru_cache); nothing crafted is stored in the repository.
CPU time of this module on one core: 75 s, 70 s of it crafting (sparse 23 s, max_k7 10 s, every other case under 7 s)."""
import functools
import math
from typing import NamedTuple

import numpy as np
import pytest

import oracle
from conftest import synth_seqs

EPS = 2.0 ** -52

# ---------------------------------------------------------------- the bands, restated from csrc/select_dev.h
FAST_BAND = 4e-7                                       # select_dev.h:110  constexpr double FAST_BAND = 4e-7
COARSE_BAND_K6 = 1.25 * 2.0**-24 * (9.0 * 12 + 7.4)  # select_dev.h coarse_band(4096)
MIN_ACCEPTS = 3
U16_MAX_WINDOWS = 32768                                # kmer_hist.hip: a longer sequence keeps the matrix at 32 bits


def coarse_band(nbins: int) -> float:
    """select_dev.h:137-139  1.25 * 0x1p-24 * (9.0 * log2(double(B)) + 7.4)"""
    return 1.25 * 2.0**-24 * (9.0 * math.log2(nbins) + 7.4)


def sel_band(nbins: int, h: float) -> float:
    """select_dev.h:85-87  4.0 * double(B) * DVS_EPS * fmax(1.0, fabs(hmean))"""
    return 4.0 * nbins * EPS * max(1.0, abs(h))


def sel_band_min(nbins: int) -> float:
    """the arbiter's band with max(1, H) at its least"""
    return sel_band(nbins, 1.0)


def near_zero_window(nbins: int) -> tuple[float, float]:
    """|margin| of a near-zero row: at least 8 x the arbiter's band at its widest (H <= log2 B), at most 0.05 x FAST_BAND"""
    return 8.0 * sel_band(nbins, math.log2(nbins)), 0.05 * FAST_BAND


# ---------------------------------------------------------------- crafting by substitution, as the k = 6 / 7 / 8 tests use it
# (test_gpu_configs.test_candidates_inside_the_f32_bands_k6, ..._fast_band_k7 and
# test_gpu_wide_rows.test_candidates_inside_the_fast_band build their streams with these two, and a stream is a
# function of their random draws: they stay as they are; band_stream below is the general form)
def _craft(oset, start, target, k, rng, tol):
    """substitutions of `start` (one to three bases at a time) until the oracle's score of the
    sequence against `oset` sits at threshold + target (records.rs:70-92) within tol.  Equal-length
    sequences give the score a grain of ~1e-8, so tol is a few of those (0.08 of the band), not zero."""
    seq = start.copy()
    thr = oset.total_jsd

    def margin(s):
        f, h = oracle.to_kfreqs(s, 4, k)
        return oset.delta_jsd(f, h) - thr

    cur = margin(seq)
    for _ in range(60_000):
        if abs(cur - target) <= tol:
            return seq, cur
        m = int(rng.integers(1, 4))
        pos = rng.integers(0, seq.size, size=m)
        old = seq[pos].copy()
        seq[pos] = (old + rng.integers(1, 4, size=m)) % 4
        d = margin(seq)
        if abs(d - target) < abs(cur - target):
            cur = d
        else:
            seq[pos] = old
    raise AssertionError(f"no sequence found at margin {target}: stuck at {cur}")


def _band_stream(k, n, length, nprefix, targets, seed):
    """a random prefix, then for every target margin a near-copy of the set's lowest member whose exact
    score is threshold + margin (each followed by a few ordinary rows), the oracle tracking the set"""
    rng = np.random.default_rng(seed)
    seqs = synth_seqs(nprefix, length, seed)
    oset = oracle.nmost(seqs, n, k, 4)
    margins = []
    for t in targets:
        labels = oset.members()[0]
        low = seqs[int(labels[oset.lowest_index])]
        cand, got = _craft(oset, low, t, k, rng, tol=0.08 * (FAST_BAND if abs(t) < 1e-6 else COARSE_BAND_K6))
        f, h = oracle.to_kfreqs(cand, 4, k)
        if oset.increases_jsd(f, h, len(seqs)):
            oset.replace_lowest(f, h, len(seqs))
        seqs.append(cand)
        margins.append(got)
        for s in synth_seqs(3, length, int(rng.integers(1 << 30))):
            f, h = oracle.to_kfreqs(s, 4, k)
            if oset.increases_jsd(f, h, len(seqs)):
                oset.replace_lowest(f, h, len(seqs))
            seqs.append(s)
    return seqs, oset, margins


MULTS = (-1.1, -0.9, -0.5, -0.1, 0.1, 0.5, 0.9, 1.1)


# ---------------------------------------------------------------- targets
class Target(NamedTuple):
    kind: str      # "fast" | "coarse": a multiple of that band; "zero": the near-zero window; "sel": a multiple of sel_band_min
    mult: float    # the multiple (zero: only its sign counts)
    band: float    # the band the margin is measured in (zero: FAST_BAND)
    lo: float      # the achieved margin must satisfy lo <= margin <= hi
    hi: float

    @property
    def goal(self):
        return 0.5 * (self.lo + self.hi)


CRAFT_TOL = 0.08  # of the band: a few grains of an equal-length row's score (see _craft)


def band_target(kind: str, mult: float, nbins: int) -> Target:
    band = {"fast": FAST_BAND, "coarse": coarse_band(nbins), "sel": sel_band_min(nbins)}[kind]
    tol = (0.1 * abs(mult) if kind == "sel" else CRAFT_TOL) * band
    return Target(kind, mult, band, mult * band - tol, mult * band + tol)


def zero_target(sign: int, nbins: int) -> Target:
    lo, hi = near_zero_window(nbins)
    return Target("zero", float(sign), FAST_BAND, lo, hi) if sign > 0 else Target("zero", float(sign), FAST_BAND, -hi, -lo)


TWO_PER_SIGN = (-0.5, 0.5)  # the B >= 8000 cases: +-0.5 x FAST_BAND and the near-zero pair (a 16384-bin score costs 4 x a 4096-bin one)


def case_targets(nbins: int, coarse: bool, two: bool) -> tuple[Target, ...]:
    out = [zero_target(-1, nbins), zero_target(1, nbins)]
    out += [band_target("fast", m, nbins) for m in (TWO_PER_SIGN if two else MULTS)]
    if coarse:
        out += [band_target("coarse", m, nbins) for m in MULTS]
    return tuple(out)


# ---------------------------------------------------------------- the oracle's run, one row at a time
class Tracker:
    """select_nmost_divergent (src/records.rs:311-342) or select_max_divergent (:390-454) replayed row by row, so that a
    row can be crafted against the set as it stands when the row arrives.  `accepts` counts the rows that changed the
    set (nmost: replace_lowest; max: a kept push or a replace_lowest at max_size) -- what the device reports as n_accepts."""

    def __init__(self, oset, mode):
        self.set, self.mode, self.accepts = oset, mode, 0

    def offer(self, f, h, label) -> bool:
        """-> the first decision (increases_jsd) for this row"""
        s = self.set
        if not s.increases_jsd(f, h, label):
            return False
        if self.mode[0] == "nmost" or s.size == self.mode[1]:
            s.replace_lowest(f, h, label)
            self.accepts += 1
            return True
        labels, _, ents, freqs = s.members(with_freqs=True)  # (clone re-runs new, records.rs:182-189)
        ns = oracle.SummedRecords.new(freqs, ents, labels)
        ns.push(f, h, label)
        stat = "std_delta_jsd" if self.mode[2] == "stdev" else "cov_delta_jsd"
        if getattr(ns, stat) > getattr(s, stat):
            self.set = ns
            self.accepts += 1
        return True

    def lowest_label(self) -> int:
        return int(self.set.members()[0][self.set.lowest_index])


STALL = 4000
PAIR_SINGLES = 2000   # single substitutions whose effect on the score is measured ...
PAIR_VERIFY = 60      # ... and pairs of them the oracle is asked about


def _craft_pair(margin, buf, n, cur, target: Target, states, k, rng):
    """Two substitutions whose effects add up to the wanted margin.  The effect of ONE substitution on the oracle's score
    is measured for up to PAIR_SINGLES positions (one score each); two substitutions that share no k-mer window and no
    bin change the score by the sum of their effects, so every substitution's best partner is looked up in the sorted
    list of effects and only the best few pairs are put to the oracle, whose answer decides.  A thousand times fewer scores than climbing needs
    where single moves are coarse (short, sparse rows).  -> the margin reached (buf changed), or None (buf as it was)."""
    pos = rng.permutation(n)[:PAIR_SINGLES]
    new = (buf[pos] + rng.integers(1, states, size=pos.size)) % states
    eff = np.empty(pos.size)
    for i, (q, b) in enumerate(zip(pos, new)):
        old, buf[q] = buf[q], b
        eff[i] = margin(n) - cur
        buf[q] = old
    order = np.argsort(eff)
    es, ps, bs = eff[order], pos[order], new[order]
    near = np.searchsorted(es, target.goal - cur - es)  # per substitution, the partner that brings the sum closest to the goal
    pairs = []
    for j in (np.clip(near, 0, es.size - 1), np.clip(near - 1, 0, es.size - 1)):
        i = np.arange(es.size)
        m = cur + es + es[j]
        ok = (j > i) & (m >= target.lo) & (m <= target.hi) & (np.abs(ps.astype(np.int64) - ps[j].astype(np.int64)) >= k)
        pairs += [(abs(m[x] - target.goal), int(x), int(j[x])) for x in np.nonzero(ok)[0]]
    for _, i, j in sorted(pairs)[:PAIR_VERIFY]:
        old = buf[ps[i]], buf[ps[j]]
        buf[ps[i]], buf[ps[j]] = bs[i], bs[j]
        m = margin(n)
        if target.lo <= m <= target.hi:
            return m
        buf[ps[i]], buf[ps[j]] = old
    return None


def _craft_seq(oset, start, target: Target, states, k, rng, max_len, tries=400_000):
    """near-copy of `start` whose oracle score against `oset` is threshold + a margin inside [target.lo, target.hi]: a
    pair of substitutions (_craft_pair); where no pair lands inside the window, hill-climbing on |margin - target.goal|
    by substituting one to three bases, appending a base or dropping the last one (a changed total moves every bin's
    frequency: a grain finer than substitutions of an equal-length row give), stopping at the FIRST margin inside."""
    buf = np.empty(max_len, dtype=np.uint8)
    n = start.size
    buf[:n] = start
    thr = oset.total_jsd

    def margin(length):
        f, h = oracle.to_kfreqs(buf[:length], states, k)
        return oset.delta_jsd(f, h) - thr

    cur = margin(n)
    got = _craft_pair(margin, buf, n, cur, target, states, k, rng)
    if got is not None:
        return buf[:n].copy(), got
    # the start is a copy of a member and scores the threshold itself: whatever the first move gives is taken, and
    # so is the next move after STALL tries without progress (a coarse-grained row has no small moves to climb with)
    dist, stall = math.inf, 0
    for _ in range(tries):
        if target.lo <= cur <= target.hi:
            return buf[:n].copy(), cur
        stall += 1
        if stall > STALL:
            dist, stall = math.inf, 0
        move = rng.random()
        if move < 0.8:
            m = int(rng.integers(1, 4))
            pos = rng.integers(0, n, size=m)
            old = buf[pos].copy()
            buf[pos] = (old + rng.integers(1, states, size=m)) % states
            d = margin(n)
            if abs(d - target.goal) < dist:
                cur, dist, stall = d, abs(d - target.goal), 0
            else:
                buf[pos] = old
        elif move < 0.9 and n < max_len:
            buf[n] = rng.integers(0, states)
            d = margin(n + 1)
            if abs(d - target.goal) < dist:
                cur, dist, stall, n = d, abs(d - target.goal), 0, n + 1
        elif n > start.size // 2:
            d = margin(n - 1)
            if abs(d - target.goal) < dist:
                cur, dist, stall, n = d, abs(d - target.goal), 0, n - 1
    raise AssertionError(f"no sequence found inside [{target.lo}, {target.hi}]: stuck at {cur}")


class Crafted(NamedTuple):
    seqs: list          # the stream (sequences), or None for a stream of frequency rows
    rows: object        # frequency rows [nrows, B] of a frequency stream, else None
    oset: object        # the oracle's set at the end of the stream (tracked row by row)
    accepts: int        # rows that changed the set
    targets: tuple      # Target per crafted row
    margins: tuple      # achieved margin per crafted row (oracle score - threshold)
    positions: tuple    # stream position per crafted row
    decisions: tuple    # the oracle's first decision (increases_jsd) per crafted row
    in_tiers: tuple     # per crafted row: the persistent scan's tiers are sure to score it (see batch_reach)


def _lengths(lengths, count, rng):
    if isinstance(lengths, int):
        return [lengths] * count
    return [int(x) for x in rng.integers(lengths[0], lengths[1] + 1, size=count)]


def _random_seqs(states, lengths, count, rng):
    return [rng.integers(0, states, size=n, dtype=np.uint8) for n in _lengths(lengths, count, rng)]


# The persistent engine's `max` works the rows behind a tentative push out in BATCHES while the set is below max_size
# (persist.hip, "BATCH: the rows behind the event"): a batch scores its rows in f64 outright, no tier sees them and
# neither rows_rechecked nor rows_coarse_passed moves.  A batch starts at an event (a row whose first decision is yes),
# holds at most P_BATCH = 32 rows, and is followed by another right away only while at least half of its rows are
# events.  Behind 48 rows that are no events no batch can reach: one that started at the last event in front of them
# holds at least 16 events and so at most 16 of them, the next holds 32 of them, no event, and ends the chain.
P_BATCH = 32
BATCH_REACH = P_BATCH // 2 + P_BATCH
QUIET_MARGIN = 1e-4  # a quiet row scores this far below the threshold: no event, and 10 x beyond every band


def wants_quiet_run(t: Target) -> bool:
    """the crafted rows of a `quiet` case that come behind BATCH_REACH quiet rows: the near-zero pair and -0.5 x both
    bands, crafted FIRST and the positive one last of them -- once a near-copy of the lowest member has been pushed, the
    lowest member is all but a duplicate, nothing scores 1e-4 below it and no quiet row can be made.  The other rows keep
    their ordinary neighbours, most of them events, and may ride in a batch."""
    return t.kind == "zero" or t.mult == -0.5


def band_stream(states, k, n, lengths, nprefix, targets, seed, mode, gap=3, quiet=False) -> Crafted:
    """A random prefix (`lengths`: one length or an inclusive range) whose first n rows seed the set, then for every
    target a near-copy of the lowest member of the set as it then stands, scored by the oracle at threshold + margin
    with the margin inside the target's window, each followed by `gap` ordinary rows.  mode: ("nmost",) or
    ("max", max_size, stat) with n the min_size; the oracle tracks the set in that mode.  quiet: the crafted rows that
    wants_quiet_run names come behind BATCH_REACH rows made of pieces of the members, which score QUIET_MARGIN and more
    below the threshold."""
    rng = np.random.default_rng(seed)
    seqs = _random_seqs(states, lengths, nprefix, rng)
    track = Tracker(oracle.SummedRecords.from_seqs(seqs[:n], k, states), mode)
    max_len = (lengths if isinstance(lengths, int) else lengths[1]) + 64

    events = [False] * n  # per stream row: the oracle's first decision

    def offer(p):
        f, h = oracle.to_kfreqs(seqs[p], states, k)
        events.append(track.offer(f, h, p))
        return events[-1]

    for p in range(n, nprefix):
        offer(p)
    margins, positions, decisions, sizes = [], [], [], []
    for t in targets:
        while quiet and wants_quiet_run(t) and any(events[-BATCH_REACH:]):
            # pieces of every member strung together: about the set's own mean, which adds nothing to its divergence
            labels = track.set.members()[0]
            size = _lengths(lengths, 1, rng)[0] // len(labels)
            s = np.concatenate([seqs[int(m)][a:a + size] for m in labels
                                for a in [int(rng.integers(0, max(1, seqs[int(m)].size - size)))]])
            f, h = oracle.to_kfreqs(s, states, k)
            if track.set.delta_jsd(f, h) - track.set.total_jsd < -QUIET_MARGIN:
                seqs.append(s)
                assert not offer(len(seqs) - 1)
        cand, got = _craft_seq(track.set, seqs[track.lowest_label()], t, states, k, rng, max_len)
        seqs.append(cand)
        margins.append(got)
        positions.append(len(seqs) - 1)
        sizes.append(mode[0] == "nmost" or track.set.size == mode[1] or not any(events[-BATCH_REACH:]))
        decisions.append(offer(len(seqs) - 1))
        for s in _random_seqs(states, lengths, gap, rng):
            seqs.append(s)
            offer(len(seqs) - 1)
    return Crafted(seqs, None, track.set, track.accepts, tuple(targets), tuple(margins), tuple(positions), tuple(decisions), tuple(sizes))


def band_stream_freqs(states, k, n, length, nprefix, targets, seed, gap=3) -> Crafted:
    """The same over frequency rows (nmost): a candidate (1 - t) f_low + t g, g an ordinary row, scores the threshold at
    t = 0 and moves continuously with t, so its margin is BISECTED against the oracle -- to any target above the
    oracle's own score noise (~1e-14 at 4096 bins).  Every row passes the reference's sum-to-one check
    (record.rs:99-104, dvs_matrix_from_freqs): oracle.entropy raises where it does not."""
    rng = np.random.default_rng(seed)

    def fresh(count):
        return [oracle.to_kfreqs(s, states, k) for s in _random_seqs(states, length, count, rng)]

    def skewed(count):
        """rows of an uneven base composition: far from the set's mean, so a step towards one RAISES the score (a step
        towards an ordinary row lowers it: the mixture is closer to the mean than the member was)"""
        p = np.arange(states, 0, -1, dtype=np.float64)
        return [oracle.to_kfreqs(rng.choice(states, size=length, p=p / p.sum()).astype(np.uint8), states, k) for _ in range(count)]

    rows, ents = map(list, zip(*fresh(nprefix)))
    track = Tracker(oracle.SummedRecords.new(np.stack(rows[:n]), ents[:n]), ("nmost",))
    for p in range(n, nprefix):
        track.offer(rows[p], ents[p], p)
    margins, positions, decisions, sizes = [], [], [], []
    for t in targets:
        oset = track.set
        thr, f_low = oset.total_jsd, rows[track.lowest_label()]

        def row_at(x, g):
            return (1.0 - x) * f_low + x * g

        def margin(x, g):
            r = row_at(x, g)
            return oset.delta_jsd(r, oracle.entropy(r)) - thr

        # a direction g and two steps along it whose margins bracket the target (a step towards an ordinary row lowers
        # the score from t = 0 on; towards a skewed row it first falls, then rises through the threshold again)
        grid = (0.0, 1e-3, 1e-2, 0.1, 0.3, 1.0)
        found = None
        for g, _ in fresh(4) + skewed(8):
            ms = [margin(x, g) for x in grid]
            for i in range(len(grid) - 1):
                if (ms[i] - t.goal) * (ms[i + 1] - t.goal) < 0 and abs(ms[i] - ms[i + 1]) > 4 * abs(t.goal):
                    found = (g, grid[i], grid[i + 1], ms[i] < t.goal)
                    break
            if found and (t.goal < 0 or found[1] > 0):
                break
        assert found, f"no direction moves the score across {t.goal}"
        g, lo_t, hi_t, rising = found
        got = None
        for _ in range(200):
            mid = 0.5 * (lo_t + hi_t)
            m = margin(mid, g)
            if t.lo <= m <= t.hi:
                got = m
                break
            if (m < t.goal) == rising:
                lo_t = mid
            else:
                hi_t = mid
        assert got is not None, f"bisection did not reach [{t.lo}, {t.hi}]"
        cand = row_at(mid, g)
        rows.append(cand)
        ents.append(oracle.entropy(cand))
        margins.append(got)
        positions.append(len(rows) - 1)
        sizes.append(True)
        decisions.append(track.offer(rows[-1], ents[-1], len(rows) - 1))
        for f, h in fresh(gap):
            rows.append(f)
            ents.append(h)
            track.offer(f, h, len(rows) - 1)
    return Crafted(None, np.stack(rows), track.set, track.accepts, tuple(targets), tuple(margins), tuple(positions),
                   tuple(decisions), tuple(sizes))


# ---------------------------------------------------------------- the cases: the smallest shapes that reach each path
class Case(NamedTuple):
    name: str
    states: int
    k: int
    mode: tuple           # ("nmost",) | ("max", max_size, stat)
    n: int                # set size (nmost) / min_size (max)
    lengths: object       # one length, or (lo, hi)
    nprefix: int
    seed: int
    count_bytes: int      # width of the count rows the build chooses (kmer_hist.hip): 2, 4; 8 = frequency rows
    coarse: bool          # the persistent instantiation has a COARSE tier for this shape (count rows, B % 256 == 0, B <= 4096)
    two: bool = False     # two targets per sign
    quiet: bool = False   # quiet runs in front of some crafted rows (band_stream)
    env: tuple = ()       # environment the case is built under
    engine: int = 1       # the engine that serves it by default (1 persistent, 0 multi-launch)
    reaches: str = ""

    @property
    def nbins(self):
        return self.states ** self.k

    @property
    def targets(self):
        return case_targets(self.nbins, self.coarse, self.two)


NMOST = ("nmost",)
# P_SMALL_ROWS = 13 (persist_dev.h): nmost 13 is the SMALL instantiation's last set size, 14 the first of OWN
SMALL13 = Case("small13", 4, 6, NMOST, 13, 5000, 300, 9101, 2, True, reaches="SMALL's last size")
OWN14 = Case("own14", 4, 6, NMOST, 14, 5000, 300, 9102, 2, True, reaches="OWN's first size")
OWN65 = Case("own65", 4, 6, NMOST, 65, 5000, 400, 9103, 2, True, reaches="OWN, a set beyond one wave's argmin")
OWN_U32 = Case("own_u32", 4, 6, NMOST, 10, 5000, 300, 9104, 4, True, env=(("DVS_COUNTS_U32", "1"),), reaches="coarse4(uint4)")
# (nmost 10 over 16-bit rows of 4096 bins is SMALL; ragged14 takes the same kind of rows to OWN)
RAGGED = Case("ragged", 4, 6, NMOST, 10, (3000, 6000), 300, 9105, 2, True, reaches="SMALL, a 1 / (T n) of its own per row")
RAGGED14 = Case("ragged14", 4, 6, NMOST, 14, (3000, 6000), 300, 9122, 2, True, reaches="OWN, a 1 / (T n) of its own per row")
# sparse: rows of 600 bases have counts of 0 and 1 only and one total, their scores lie on a lattice too coarse for the
# near-zero window (400 000 moves ended 3.4e-6 away); 1000 bases (61 % of sl's bins still zero with a set of 3) reach
# it, at ~4 s per FAST-sized target: hence two FAST targets per sign
SPARSE = Case("sparse", 4, 6, NMOST, 3, 1000, 300, 9106, 2, True, two=True, reaches="zero bins of sl (1e-30), the <= eps -> 0 clamps")
K5 = Case("k5", 4, 5, NMOST, 10, 3000, 300, 9107, 2, True, reaches="coarse_band(1024)")
# 64 bins: B & 255 != 0, so p_scan_rows and p_scan_rows_wg have no COARSE tier for it on any path (FAST targets only)
K3 = Case("k3", 4, 3, NMOST, 10, 3000, 300, 9108, 2, False, reaches="the scalar FAST loop at 64 bins")
PROT400 = Case("prot400", 20, 2, NMOST, 7, 2000, 300, 9109, 2, False, reaches="rolled index, B = 400")
ODD125 = Case("odd125", 5, 3, NMOST, 7, 2000, 300, 9110, 4, False, reaches="B % 4 != 0: 32-bit rows, scalar tails")
BIG8000 = Case("big8000", 20, 3, NMOST, 8, 5000, 200, 9111, 4, False, two=True, reaches="not-cached instantiation, B != 4^7")
MAX_K6 = tuple(Case(f"max_k6_{stat}", 4, 6, ("max", 40, stat), 5, 5000, 300, 9112 + i, 2, True, quiet=True,
                    reaches="persist_nmost_kernel<T, true, true>, batches") for i, stat in enumerate(("stdev", "cov")))
MAX_K4 = tuple(Case(f"max_k4_{stat}", 4, 4, ("max", 40, stat), 5, 3000, 300, 9114 + i, 2, True, quiet=True,
                    reaches="the same at 256 bins") for i, stat in enumerate(("stdev", "cov")))
MAX_K7 = Case("max_k7", 4, 7, ("max", 20, "stdev"), 4, 5000, 150, 9116, 4, False, two=True, engine=0,
              reaches="multi-launch max_batch_* kernels")
FREQS_K6 = Case("freqs_k6", 4, 6, NMOST, 10, 5000, 300, 9117, 8, False, reaches="FAST on T = double, exact margins")
ARBITER_MULTS = (0.25, 3.0)  # x sel_band_min(4096), both signs: inside the arbiter's band, and at its edge region
ARBITER_K6 = tuple(Case(f"arbiter_k6_{m}", 4, 6, NMOST, 10, 5000, 300, 9118 + i, 8, False,
                        reaches="the edge of sel_band") for i, m in enumerate(ARBITER_MULTS))

B4096_COUNT_CASES = (SMALL13, OWN14, OWN65, OWN_U32, RAGGED, RAGGED14)
OTHER_SEQ_CASES = (SPARSE, K5, K3, PROT400, ODD125, BIG8000) + MAX_K6 + MAX_K4 + (MAX_K7,)
SEQ_CASES = B4096_COUNT_CASES + OTHER_SEQ_CASES
FREQ_CASES = (FREQS_K6,) + ARBITER_K6
ALL_CASES = SEQ_CASES + FREQ_CASES

# head phase (a device-resident build of >= 17 408 rows is split at row 1024, kmer_hist.hip): the small13 stream and
# one whose six crafted rows sit at positions 1020, 1022, .. 1030, each followed by short ordinary rows up to HEAD_ROWS
HEAD_SPLIT_AT = 1024
HEAD_ROWS = 17_600
HEAD_FILL_LENGTH = 260
STRADDLE = SMALL13._replace(name="straddle", nprefix=1020, seed=9121)
STRADDLE_GAP = 1


def straddle_targets():
    B = STRADDLE.nbins
    return (zero_target(-1, B), zero_target(1, B), band_target("fast", -0.5, B), band_target("fast", 0.5, B),
            band_target("coarse", -0.5, B), band_target("coarse", 0.5, B))


def _arbiter_targets(case: Case):
    m = ARBITER_MULTS[ARBITER_K6.index(case)]
    return (band_target("sel", -m, case.nbins), band_target("sel", m, case.nbins))


@functools.lru_cache(maxsize=None)
def crafted(case: Case) -> Crafted:
    if case in ARBITER_K6:
        return band_stream_freqs(case.states, case.k, case.n, case.lengths, case.nprefix, _arbiter_targets(case), case.seed)
    if case.count_bytes == 8:
        return band_stream_freqs(case.states, case.k, case.n, case.lengths, case.nprefix, case.targets, case.seed)
    if case is STRADDLE:
        return band_stream(case.states, case.k, case.n, case.lengths, case.nprefix, straddle_targets(), case.seed, case.mode,
                           gap=STRADDLE_GAP)
    targets = sorted(case.targets, key=lambda t: (not wants_quiet_run(t), t.mult > 0)) if case.quiet else case.targets
    return band_stream(case.states, case.k, case.n, case.lengths, case.nprefix, targets, case.seed, case.mode,
                       quiet=case.quiet)


@functools.lru_cache(maxsize=None)
def head_stream(case: Case):
    """(sequences, the oracle's set, its accept count): the crafted stream of `case` followed by short ordinary rows up to
    HEAD_ROWS, so that a device-resident build splits and the persistent engine walks the first 1024 rows on the head CUs"""
    c = crafted(case)
    fill = synth_seqs(HEAD_ROWS - len(c.seqs), HEAD_FILL_LENGTH, case.seed + 50, ragged=True)
    seqs = list(c.seqs) + fill
    exp, acc = oracle.nmost_concat(*oracle.concat(seqs), case.n, case.k, case.states)
    return seqs, exp, acc


@functools.lru_cache(maxsize=None)
def oracle_whole(case: Case):
    """the oracle's own run over the finished stream (C, start to end): (set, accept count or None for max)"""
    c = crafted(case)
    if c.rows is not None:
        return oracle.final_nmost(c.rows, case.n), None
    if case.mode[0] == "nmost":
        return oracle.nmost_concat(*oracle.concat(c.seqs), case.n, case.k, case.states)
    return oracle.max_divergent(c.seqs, case.n, case.mode[1], case.k, case.states, case.mode[2]), None


def in_units(c: Crafted):
    """achieved margins in units of their band, for the device tests' print-outs"""
    return [f"{t.kind}:{m / t.band:+.4f}" for t, m in zip(c.targets, c.margins)]


def sure_within(c: Crafted, kind_band: float, tiers_only: bool = False) -> int:
    """crafted rows whose margin is within 0.6 x the band: the tier of that band may not decide them.  tiers_only: of
    those, the rows no batch of the persistent `max` can reach (in_tiers): a full set, or BATCH_REACH quiet rows in front"""
    return sum(1 for m, t in zip(c.margins, c.in_tiers) if abs(m) <= 0.6 * kind_band and (t or not tiers_only))


_ids = lambda c: c.name  # noqa: E731


# ------------------------------------------------------------------------------------------------ the tests
def test_the_bands_are_those_of_select_dev_h():
    assert coarse_band(4096) == COARSE_BAND_K6
    assert abs(coarse_band(4096) - 8.6e-6) < 1e-7 and coarse_band(1024) < coarse_band(4096) < coarse_band(8192)
    assert FAST_BAND == 4e-7
    assert sel_band_min(4096) == 4 * 4096 * 2.0 ** -52 and abs(sel_band_min(4096) - 3.64e-12) < 1e-14
    for case in ALL_CASES:
        lo, hi = near_zero_window(case.nbins)
        assert 8 * sel_band(case.nbins, math.log2(case.nbins)) == lo < 0.25 * hi and hi == 0.05 * FAST_BAND


def test_every_case_of_the_table_is_there():
    by = {c.name: c for c in ALL_CASES}
    assert len(by) == len(ALL_CASES)
    shape = {name: (c.states, c.k, c.nbins, c.mode, c.n, c.count_bytes) for name, c in by.items()}
    assert shape["small13"] == (4, 6, 4096, NMOST, 13, 2) and shape["own14"] == (4, 6, 4096, NMOST, 14, 2)
    assert shape["own65"] == (4, 6, 4096, NMOST, 65, 2) and shape["own_u32"] == (4, 6, 4096, NMOST, 10, 4)
    assert by["own_u32"].env == (("DVS_COUNTS_U32", "1"),)
    assert shape["ragged"] == (4, 6, 4096, NMOST, 10, 2) and by["ragged"].lengths == (3000, 6000)
    assert shape["sparse"] == (4, 6, 4096, NMOST, 3, 2) and by["sparse"].lengths == 1000
    assert shape["k5"] == (4, 5, 1024, NMOST, 10, 2) and shape["k3"] == (4, 3, 64, NMOST, 10, 2)
    assert shape["prot400"] == (20, 2, 400, NMOST, 7, 2) and shape["odd125"] == (5, 3, 125, NMOST, 7, 4)
    assert shape["big8000"] == (20, 3, 8000, NMOST, 8, 4) and by["big8000"].two
    for stat in ("stdev", "cov"):
        assert shape[f"max_k6_{stat}"] == (4, 6, 4096, ("max", 40, stat), 5, 2)
        assert shape[f"max_k4_{stat}"] == (4, 4, 256, ("max", 40, stat), 5, 2)
    assert shape["max_k7"] == (4, 7, 16384, ("max", 20, "stdev"), 4, 4) and by["max_k7"].two and by["max_k7"].engine == 0
    assert shape["freqs_k6"] == (4, 6, 4096, NMOST, 10, 8)
    assert [shape[f"arbiter_k6_{m}"] for m in ARBITER_MULTS] == [(4, 6, 4096, NMOST, 10, 8)] * 2
    for c in ALL_CASES:
        assert 150 <= c.nprefix <= 700
        assert c.engine == (0 if c is MAX_K7 else 1)
    assert STRADDLE.nprefix + STRADDLE_GAP * 2 * 2 == HEAD_SPLIT_AT  # (crafted rows on both sides of the hand-over)


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids)
def test_shapes_take_the_intended_branch(case):
    B = case.nbins
    cached = B <= 4096                                  # persist_dev.h: P_J * P_THREADS bins in the register cache
    u16 = B <= 4096 and B % 4 == 0 and not case.env     # kmer_hist.hip: 16-bit rows (DVS_COUNTS_U32 keeps 32)
    if case.count_bytes != 8:
        assert case.count_bytes == (2 if u16 else 4)
        hi = case.lengths if isinstance(case.lengths, int) else case.lengths[1]
        assert hi + 64 - case.k + 1 <= U16_MAX_WINDOWS  # (crafting may append up to 64 bases)
    # COARSE: count rows whose state fits the register cache, in the 256-bin vector loop of p_scan_rows
    assert case.coarse == (case.count_bytes != 8 and cached and B % 256 == 0)
    if case.mode[0] == "max":
        assert (case.engine == 1) == cached             # dvs_persist_setup: `max` beyond the cache is the multi-launch engine's
    if case is ODD125:
        assert B % 4 == 1 and B % 64 != 0
    if case is BIG8000:
        assert 4096 < B <= 16384 and B != 4 ** 7 and B % 256 != 0
    if case in (SMALL13, OWN14):
        assert (case.n <= 13) == (case is SMALL13)      # P_SMALL_ROWS
    if case is OWN65:
        assert case.n > 64
    kinds = [t.kind for t in (case.targets if case not in ARBITER_K6 else _arbiter_targets(case))]
    if case in ARBITER_K6:
        assert kinds == ["sel", "sel"]
    else:
        assert kinds.count("zero") == 2 and kinds.count("fast") == (2 if case.two else 8)
        assert kinds.count("coarse") == (8 if case.coarse else 0)


def _check_crafted(case, c: Crafted, whole):
    assert len(c.margins) == len(c.targets) and not any(m is None for m in c.margins)  # (no target dropped)
    lo0, hi0 = near_zero_window(case.nbins)
    for t, m, dec in zip(c.targets, c.margins, c.decisions):
        assert t.lo <= m <= t.hi, (t, m)
        if t.kind == "zero":
            assert lo0 <= abs(m) <= hi0 and (m > 0) == (t.mult > 0), (t, m)
        elif t.kind == "sel":
            assert abs(m - t.mult * t.band) <= 0.1 * abs(t.mult) * t.band
        else:
            assert abs(m - t.mult * t.band) <= CRAFT_TOL * t.band < 0.6 * t.band
        assert dec == (m > 0), (t, m, dec)               # (the oracle accepts exactly the rows above the threshold)
    exp, acc = whole
    assert exp.members()[0].tolist() == c.oset.members()[0].tolist()  # (the tracked set is the stream's)
    if acc is not None:
        assert acc == c.accepts
    assert c.accepts >= MIN_ACCEPTS
    if c.rows is not None:
        assert len({r.tobytes() for r in c.rows}) == len(c.rows)
    else:
        assert len({s.tobytes() for s in c.seqs}) == len(c.seqs)
        assert max(s.size for s in c.seqs) - case.k + 1 <= U16_MAX_WINDOWS
    signs = [m > 0 for t, m in zip(c.targets, c.margins) if t.kind in ("zero", "sel")]
    assert sorted(signs) == [False, True]                # (the near-zero / arbiter pair: one row of each sign)


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids)
def test_crafted_rows_sit_where_they_were_aimed(case):
    _check_crafted(case, crafted(case), oracle_whole(case))


def test_the_straddling_stream_and_the_head_fill():
    c = crafted(STRADDLE)
    exp, acc = oracle.nmost_concat(*oracle.concat(c.seqs), STRADDLE.n, STRADDLE.k, STRADDLE.states)
    _check_crafted(STRADDLE, c, (exp, acc))
    assert list(c.positions) == [1020, 1022, 1024, 1026, 1028, 1030]
    assert min(c.positions) < HEAD_SPLIT_AT <= max(c.positions)
    assert max(crafted(SMALL13).positions) < HEAD_SPLIT_AT
    for case in (SMALL13, STRADDLE):
        seqs, exp, acc = head_stream(case)
        assert len(seqs) == HEAD_ROWS and HEAD_ROWS - HEAD_SPLIT_AT >= 16 * HEAD_SPLIT_AT  # (kmer_hist.hip: the build splits)
        assert acc >= crafted(case).accepts
