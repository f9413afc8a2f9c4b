"""Input families for the oldest stage entry points (k_lts_batch, k_symfront_batch, k_ptrack_batch, k_demap_batch, k_deint_batch behind sora_hip_lts11a,
_symfront11a, _pilot_track11a, _pilot11a, _demap11a, _deinterleave11a) and for the thin 802.11n rows (demap11n, sig_demap11n, siso_est11n, mimo_est11n):
rails, zeros, nulls, wraps and tile edges.  Deterministic from the seeds below, numpy only; tests/test_stage_edges_cpu.py pins the oracle to the reference's own
bricks on these families (live and from tests/golden/ref_vectors_11a_stages.npz), tests/test_gpu_stage_edges.py pins the kernels to the oracle.

Where a family starts from a signal (the transmitter's L-LTF, the equalised symbols of a frame) the caller hands in the oracle (oracle.pyoracle.Oracle); everything
else is drawn from numpy's generator."""
import numpy as np

SEED_LTS, SEED_SYM, SEED_CTX, SEED_TRACK, SEED_DEMAP, SEED_DEINT, SEED_11N = 7101, 7102, 7103, 7104, 7105, 7106, 7107

RAILS = np.array([-32768, 32767], np.int16)
USED = np.array([b for b in range(64) if 1 <= b <= 26 or b >= 38])             # the bins _build_coeff / _rotate define (pilot.hpp:137-164)
PILOTS = (7, 21, 43, 57)
DATA48 = np.array([b for b in list(range(38, 64)) + list(range(1, 27)) if b not in PILOTS])   # T11aDemap's carrier order (demapper11a.hpp:21-37)

LTS_ROWS = (1, 2, 63, 64, 65)                                                   # one frame per block
SYMFRONT_ROWS = (1, 15, 16, 17, 63, 64, 65, 1003)                               # 16 symbols per tile, 4 tiles per block
DEMAP_ROWS = (1, 31, 32, 33, 257)                                               # 32 symbols per tile
TRACK_NSYM = (0, 1, 2, 126, 127, 128, 254, 300)
START_COUNTS = (0, 1, 125, 126, 127)


def _uniform(rng, amp, shape):
    return rng.integers(-amp, amp + 1, size=shape).astype(np.int16)


def _full(rng, shape):
    return rng.integers(-32768, 32768, size=shape).astype(np.int16)


def _rails(rng, shape):
    return RAILS[rng.integers(0, 2, size=shape)]


def _clip16(z):
    return np.stack([np.clip(np.rint(z.real), -32768, 32767), np.clip(np.rint(z.imag), -32768, 32767)], -1).astype(np.int16)


def _cplx(x):
    return x[..., 0].astype(np.float64) + 1j * x[..., 1]


# ---------------------------------------------------------------------------------------------- context records
def lts_record(ctx):
    """RxCtx -> the 258 int16 of sora_lts11a_ctx: cfo_est, reserved, freq[64][2], chan[64][2]"""
    return np.concatenate([[ctx.CFO_est, 0], np.array(ctx.FreqCoeffs[:], np.int16), np.array(ctx.ChannelCoeffs[:], np.int16)]).astype(np.int16)


def state_record(ctx):
    """RxCtx -> the 134 int16 of sora_track11a_state: cfo_comp, sfo_comp, cfo_tracker, sfo_tracker, symbol_count (uint32), comp[64][2]"""
    r = np.zeros(134, np.int16)
    r[0], r[1], r[2], r[3] = ctx.CFO_comp, ctx.SFO_comp, ctx.CFO_tracker, ctx.SFO_tracker
    r[4:6] = np.array([ctx.symbol_count], np.uint32).view(np.int16)
    r[6:] = np.array(ctx.CompCoeffs[:], np.int16)
    return r


def put_lts_record(ctx, rec):
    ctx.CFO_est = int(rec[0])
    ctx.FreqCoeffs[:] = [int(v) for v in rec[2:130]]
    ctx.ChannelCoeffs[:] = [int(v) for v in rec[130:258]]
    return ctx


def put_state_record(ctx, rec):
    ctx.CFO_comp, ctx.SFO_comp, ctx.CFO_tracker, ctx.SFO_tracker = (int(v) for v in rec[:4])
    ctx.symbol_count = int(np.ascontiguousarray(rec[4:6]).view(np.uint32)[0])
    ctx.CompCoeffs[:] = [int(v) for v in rec[6:]]
    return ctx


def reset_state():
    """the record of a context after Reset (ieee80211facade.hpp:190-221): CompCoeffs = 0x7fff, symbol_count = 127"""
    r = np.zeros(134, np.int16)
    r[4] = 127; r[6::2] = 0x7fff
    return r


# ---------------------------------------------------------------------------------------------- L-LTF inputs [n, 144, 2]
def tx_preamble20(oracle):
    """-> (the transmitter's own 6 Mbps frame at 20 MHz as complex float, index of the 144 samples the receive graph hands T11aLTS)"""
    cap = oracle.tx_capture(bytes(range(40)), 6000, lead=64, rate_mhz=20)
    res = oracle.rx_capture(cap, 20)
    assert len(res) == 1 and res[0]["length"] == 44
    return _cplx(cap) / 256.0, int(res[0]["start_sample"])


COHERENT_ANGLES = (0.0, np.pi / 2, -np.pi / 2, np.pi * (1 - 1 / 1024), np.pi, -np.pi * (1 - 1 / 1024), -np.pi)
ROTATION_TURNS = (-1.02, -1.001, -0.999, -0.98, -0.75, -0.5, -0.25, -0.02, 0.0, 0.02, 0.25, 0.5, 0.75, 0.98, 0.999, 1.001, 1.02)   # x pi over 64 samples


def lts_cases(oracle):
    """-> (names, x int16 [n, 144, 2])"""
    names, xs = [], []

    def add(name, x):
        names.append(name); xs.append(np.ascontiguousarray(x, np.int16).reshape(144, 2))
    rng = np.random.default_rng(SEED_LTS)
    add("zero", np.zeros((144, 2)))
    add("const+", np.full((144, 2), 32767)); add("const-", np.full((144, 2), -32768))
    add("const-+", np.tile(np.array([-32768, 32767]), (144, 1)))
    for i in range(4):
        add("rails%d" % i, _rails(rng, (144, 2)))
    for i in range(6):
        add("full%d" % i, _full(rng, (144, 2)))
    for k in range(16):                                                          # 1, 2, 4 ... 16384, 32767
        for j in range(2):
            add("amp%d_%d" % (min(1 << k, 32767), j), _uniform(rng, min(1 << k, 32767), (144, 2)))
    z, s = tx_preamble20(oracle)
    w = z[s:s + 144]; peak = max(np.abs(w.real).max(), np.abs(w.imag).max())
    for lvl in (30, 400, 8000, 32767, 65534):                                    # the last one clips
        add("tx_level%d" % lvl, _clip16(w * (lvl / peak)))
    n = np.arange(144)
    for t in ROTATION_TURNS:                                                     # the two halves differ by t x pi: CFO_est over its whole range, both sides of +-pi
        add("tx_turn%+.3f" % t, _clip16(w * (8000 / peak) * np.exp(1j * np.pi * t * n / 64)))
    for i in range(12):                                                          # an echo within 1 dB of the direct path: single bins null
        d = 1 + i % 3
        a = 10 ** (rng.uniform(-1, 1) / 20) * np.exp(1j * rng.uniform(-np.pi, np.pi))
        y = z[s:s + 144] + a * z[s - d:s - d + 144]
        add("tx_echo%d" % i, _clip16(y * (12000 / max(np.abs(y.real).max(), np.abs(y.imag).max()))))
    for kind in ("min", "rails", "full"):                                        # coherent full scale: second half = first half turned by one angle
        for ai, ang in enumerate(COHERENT_ANGLES):
            x = _full(rng, (144, 2))
            if kind == "min":
                x[8:72] = -32768
            elif kind == "rails":
                x[8:72] = _rails(rng, (64, 2))
            x[72:136] = _clip16(_cplx(x[8:72]) * np.exp(1j * ang))
            add("coherent_%s_%d" % (kind, ai), x)
    return names, np.stack(xs)


def lts_sums(x):
    """FreqOffsetEstimate's two 64-term sums (dspalg.hpp:226-243) in exact integers (int64), before any 32-bit wrap: x int16 [n, 144, 2] -> (re, im) int64 [n]"""
    x = x.astype(np.int64)
    a = x[:, 8:72] >> 1; b = x[:, 72:136]
    re = b[..., 0] * a[..., 0] + b[..., 1] * a[..., 1]
    im = b[..., 1] * a[..., 0] - b[..., 0] * a[..., 1]
    return (re >> 5).sum(1), (im >> 5).sum(1)


def wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


# ---------------------------------------------------------------------------------------------- symbols for the symbol front end [n, 80, 2]
def symfront_symbols(n=1003):
    rng = np.random.default_rng(SEED_SYM)
    x = np.zeros((n, 80, 2), np.int16)
    for i in range(n):
        k = i % 7
        if k == 1:
            x[i] = _rails(rng, (80, 2))
        elif k == 2:
            x[i] = _full(rng, (80, 2))
        elif k == 3:
            x[i] = _uniform(rng, 30, (80, 2))
        elif k == 4:
            x[i] = ((32767, 32767), (-32768, -32768), (-32768, 32767))[(i // 7) % 3]
        elif k == 5:
            x[i] = _uniform(rng, 32767, (80, 2))
        elif k == 6:
            x[i] = _uniform(rng, 3000, (80, 2))
    return x                                                                     # k == 0: zero


def random_ctx_records(m=8):
    """full-range coefficient sets, rails included: int16 [m, 258]"""
    rng = np.random.default_rng(SEED_CTX)
    c = _full(rng, (m, 258)); c[:, 1] = 0
    c[0, 2:] = 32767; c[1, 2:] = -32768; c[2, 2:] = _rails(rng, (256,))
    c[3, 2:130] = -32768; c[4, 130:] = -32768
    return c


def symfront_index(n, m):
    """ctx_index: unsorted, with repeats, every set used"""
    rng = np.random.default_rng(SEED_CTX + 1)
    idx = rng.integers(0, m, n).astype(np.int32)
    if n >= m:
        idx[rng.permutation(n)[:m]] = np.arange(m)
    return idx


# ---------------------------------------------------------------------------------------------- tracker frames
def frame_eq_symbols(oracle, nsym=300):
    """the oracle's own equalised symbols (SIGNAL first) of one 6 Mbps frame of at least `nsym` symbols, a little noise and carrier offset on it"""
    rng = np.random.default_rng(SEED_TRACK + 1)
    mp = rng.integers(0, 256, 3 * nsym + 4, dtype=np.uint8).tobytes()
    cap = oracle.tx_capture(mp, 6000, lead=40, rate_mhz=20)
    z = _cplx(cap) * np.exp(2j * np.pi * 21e3 * np.arange(len(cap)) / 20e6) + rng.normal(0, 120, len(cap)) + 1j * rng.normal(0, 120, len(cap))
    cap = _clip16(z)
    res = oracle.rx_capture(cap, 20)
    assert len(res) == 1 and res[0]["nsym"] >= nsym, res
    s = res[0]["start_sample"]
    ctx = oracle.new_ctx(); oracle.lts(ctx, cap[s:s + 144])
    return np.stack([oracle.sym_front(ctx, cap[s + 144 + 80 * k:s + 224 + 80 * k]) for k in range(nsym)])


TRACK_KINDS = ("frame", "full", "rails", "zero", "pilots")


def track_frames(oracle):
    """-> dict: eq int16 [total, 64, 2]; first, nsym int32 [f] (unsorted, with gaps between the frames); state0 int16 [f, 134]; kind [f].
    Frame f = kind f // 8 with TRACK_NSYM[f % 8] symbols.  Every third frame starts from the reset state, the others from arbitrary records: full-range cfo_comp,
    sfo_comp, cfo_tracker, sfo_tracker, symbol_count cycling through START_COUNTS, comp[] full range with -32768 present."""
    rng = np.random.default_rng(SEED_TRACK)
    feq = frame_eq_symbols(oracle, max(TRACK_NSYM))
    nf = len(TRACK_KINDS) * len(TRACK_NSYM)
    nsym = np.array([TRACK_NSYM[f % len(TRACK_NSYM)] for f in range(nf)], np.int32)
    kind = [TRACK_KINDS[f // len(TRACK_NSYM)] for f in range(nf)]
    first = np.zeros(nf, np.int32); pos = 0
    for f in rng.permutation(nf):
        pos += int(rng.integers(0, 4)); first[f] = pos; pos += int(nsym[f])
    total = pos + 3
    eq = _full(rng, (total, 64, 2))                                              # the gaps hold data too: a kernel that strays into them shows
    state0 = np.zeros((nf, 134), np.int16); k = 0
    for f in range(nf):
        a, b = int(first[f]), int(first[f] + nsym[f])
        if kind[f] == "frame":
            eq[a:b] = feq[:nsym[f]]
        elif kind[f] == "rails":
            eq[a:b] = _rails(rng, (b - a, 64, 2))
        elif kind[f] == "zero":
            eq[a:b] = 0
        elif kind[f] == "pilots":
            p = eq[a:b, PILOTS].copy(); eq[a:b] = 0; eq[a:b, PILOTS] = p
        if f % 3 == 0:
            state0[f] = reset_state()
        else:
            st = _full(rng, (134,))
            st[4:6] = np.array([START_COUNTS[k % len(START_COUNTS)]], np.uint32).view(np.int16); k += 1
            st[6 + 2 * (f % 64):8 + 2 * (f % 64)] = -32768
            if f % 7 == 1:
                st[6:] = -32768
            state0[f] = st
    return {"eq": eq, "first": first, "nsym": nsym, "state0": state0, "kind": kind}


def start_count(state):
    return int(np.ascontiguousarray(state[4:6]).view(np.uint32)[0])


def count_wraps(c0, n):
    """how often symbol_count goes 126 -> 0 in n symbols from c0 (pilot.hpp:186-187: count++, then 0 once it reaches 127)"""
    w = 0; c = c0
    for _ in range(n):
        w += c == 126
        c = 0 if c + 1 >= 127 else c + 1
    return w


# ---------------------------------------------------------------------------------------------- demap / de-interleave
CLAMP_VALUES = np.array([16 * k + d for k in range(-132, 133) for d in (-1, 0, 1)], np.int16)        # +-2100 and a little: re >> 4 = -128 / 127 straddled


def demap_symbols(n=257):
    rng = np.random.default_rng(SEED_DEMAP)
    x = _full(rng, (n, 64, 2))
    rows = -(-len(CLAMP_VALUES) // 48)                                           # 17 symbols hold every value once in re and once in im of a data carrier
    v = np.resize(CLAMP_VALUES, rows * 48).reshape(rows, 48)
    x[:rows, DATA48, 0] = v
    x[:rows, DATA48, 1] = np.roll(v.ravel(), 397).reshape(rows, 48)
    x[rows] = 32767; x[rows + 1] = -32768; x[rows + 2] = _rails(rng, (64, 2)); x[rows + 3, :, 0] = -32768; x[rows + 3, :, 1] = 32767
    return x


def deint_bytes(nb, n=257):
    """rows 0 and 1: the positions 0 .. 48 nb - 1 as two byte planes (the permutation itself); the rest random bytes"""
    rng = np.random.default_rng(SEED_DEINT + nb)
    s = rng.integers(0, 256, size=(n, 48 * nb)).astype(np.uint8)
    if n >= 2:
        idx = np.arange(48 * nb); s[0] = idx & 0xFF; s[1] = idx >> 8
    return s


# ---------------------------------------------------------------------------------------------- 802.11n
def demap11n_symbols(n=257):
    rng = np.random.default_rng(SEED_11N)
    x = _full(rng, (n, 64, 2))
    x[n // 2:n // 2 + 40] = _rails(rng, (40, 64, 2)); x[3] = 32767; x[4] = -32768; x[5, :, 0] = -32768; x[5, :, 1] = 32767
    v = np.resize(CLAMP_VALUES, 17 * 64).reshape(17, 64)
    x[8:25, :, 0] = v; x[8:25, :, 1] = np.roll(v.ravel(), 397).reshape(17, 64)
    return x


def sig_demap11n_symbols(n=65):
    rng = np.random.default_rng(SEED_11N + 1)
    x = _full(rng, (n, 3, 64, 2))
    x[n // 2:n // 2 + 12] = _rails(rng, (12, 3, 64, 2)); x[3] = 32767; x[4] = -32768; x[5] = 0
    return x


def siso_est11n_lltfs():
    """-> (l0, l1) int16 [n, 128, 2]: both chains at full scale, on the rails, at zero, one chain zero"""
    rng = np.random.default_rng(SEED_11N + 2)
    n = 36
    l0 = _full(rng, (n, 128, 2)); l1 = _full(rng, (n, 128, 2))
    l0[8:16] = _rails(rng, (8, 128, 2)); l1[8:16] = _rails(rng, (8, 128, 2))
    l0[16] = 32767; l1[16] = 32767; l0[17] = -32768; l1[17] = -32768; l0[18] = 32767; l1[18] = -32768
    l0[19] = 0; l1[19] = 0
    l0[20:24] = 0; l1[24:28] = 0
    l0[28:30] = 0; l1[28:30] = _rails(rng, (2, 128, 2)); l1[30:32] = 0; l0[30:32] = _rails(rng, (2, 128, 2))
    return l0, l1


SINGULAR_COUNTS = (1, 5, 20, 40, 55)


def mimo_est11n_ltfs():
    """-> (l0, l1) int16 [n, 128, 2]: zero, rails, one chain zero, l1 = +-l0 on a subset of carriers only (both HT-LTF symbols), amplitudes 1 .. 3"""
    rng = np.random.default_rng(SEED_11N + 3)
    n = 44
    l0 = _uniform(rng, 32767, (n, 128, 2)); l1 = _uniform(rng, 32767, (n, 128, 2))
    l0[0] = 0; l1[0] = 0
    l0[1:5] = _rails(rng, (4, 128, 2)); l1[1:5] = _rails(rng, (4, 128, 2))
    l0[5] = 32767; l1[5] = 32767; l0[6] = -32768; l1[6] = -32768; l0[7] = -32768; l1[7] = 32767
    l0[8:11] = 0; l1[11:14] = 0
    f = 14
    for amp in (32767, 3000, 300):
        for k in SINGULAR_COUNTS:
            l0[f] = _uniform(rng, amp, (128, 2)); l1[f] = _uniform(rng, amp, (128, 2))
            bins = rng.permutation(64)[:k]; sgn = rng.choice([-1, 1], k)
            for b, s in zip(bins, sgn):
                l1[f, b] = s * l0[f, b]; l1[f, b + 64] = s * l0[f, b + 64]
            f += 1
    for amp in (1, 2, 3):
        for _ in range(5):
            l0[f] = _uniform(rng, amp, (128, 2)); l1[f] = _uniform(rng, amp, (128, 2)); f += 1
    assert f == n
    return l0, l1


def mimo_singular_carriers(l0, l1):
    """per frame, the number of carriers whose 2x2 channel has determinant exactly 0, in exact integers (channel_11n.hpp:329-443: h = ((p - q) >> 1, (p + q) >> 1)
    per chain with saturating 16-bit sums; a common sign does not matter to det == 0)"""
    sat = lambda v: np.clip(v, -32768, 32767)                                    # noqa: E731
    h = []
    for l in (l0.astype(np.int64), l1.astype(np.int64)):
        p, q = l[:, :64], l[:, 64:]
        h.append((sat(p - q) >> 1, sat(p + q) >> 1))
    cm = lambda a, b: (a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0])   # noqa: E731
    ad = cm(h[0][0], h[1][1]); bc = cm(h[0][1], h[1][0])
    return ((ad[0] == bc[0]) & (ad[1] == bc[1])).sum(1)


# ---------------------------------------------------------------------------------------------- the families through a CPU engine (the oracle or the reference's bricks)
class Engine:
    """lts(ctx, in144), sym_front(ctx, in80) -> eq, sym_track(ctx, eq) -> out over oracle.pyoracle.RxCtx: the oracle's stage functions or the reference's own bricks"""
    def __init__(self, oracle, graph=None):
        self.new_ctx = oracle.new_ctx
        if graph is None:
            self.lts, self.sym_front, self.sym_track = oracle.lts, oracle.sym_front, oracle.sym_track
        else:
            self.lts, self.sym_front, self.sym_track = graph.lts11a, graph.sym_front11a, graph.sym_track11a


def run_lts(e, x):
    """-> (records int16 [n, 258], what the brick left in CFO_comp, SFO_comp, CFO_tracker, SFO_tracker [n, 4]); the four start non-zero: T11aLTS clears them"""
    rec, post = [], []
    for i in range(len(x)):
        c = e.new_ctx(); c.CFO_comp, c.SFO_comp, c.CFO_tracker, c.SFO_tracker = 11, -12, 13, -14
        e.lts(c, x[i])
        rec.append(lts_record(c)); post.append([c.CFO_comp, c.SFO_comp, c.CFO_tracker, c.SFO_tracker])
    return np.stack(rec), np.array(post, np.int16)


def run_symfront(e, x, ctx_records, idx):
    ctxs = [put_lts_record(e.new_ctx(), r) for r in ctx_records]
    return np.stack([e.sym_front(ctxs[idx[i]], x[i]) for i in range(len(x))])


def run_track(e, fr, frames=None):
    """-> (out int16 [total, 64, 2]: the USED bins of every tracked symbol, zero elsewhere and outside the frames; state after every symbol int16 [total, 134];
    state at the end of every frame int16 [f, 134] -- the start state where a frame is empty or not in `frames`)"""
    out = np.zeros_like(fr["eq"]); states = np.zeros((len(fr["eq"]), 134), np.int16); end = fr["state0"].copy()
    for f in (range(len(fr["first"])) if frames is None else frames):
        c = put_state_record(e.new_ctx(), fr["state0"][f])
        for s in range(int(fr["first"][f]), int(fr["first"][f] + fr["nsym"][f])):
            w = e.sym_track(c, fr["eq"][s])
            out[s][USED] = w[USED]; states[s] = state_record(c)
        end[f] = state_record(c)
    return out, states, end


# ---------------------------------------------------------------------------------------------- the recorded subset (tests/golden/ref_vectors_11a_stages.npz)
REC_SYM_ROWS, REC_ROWS, REC_TRACK_NSYM = 129, 33, (1, 2, 128)
SEEDS = np.array([SEED_LTS, SEED_SYM, SEED_CTX, SEED_TRACK, SEED_DEMAP, SEED_DEINT, SEED_11N], np.int64)


def cpu_functions(oracle, graph=None, kernels=None):
    """the per-symbol functions of the oracle, or (graph = ReferenceGraph, kernels = Reference) of the compiled reference"""
    if graph is None:
        return {"demap": oracle.demap, "deinterleave": oracle.deinterleave, "demap11n": oracle.demap11n, "sig_demap11n": oracle.sig_demap11n,
                "siso_est11n": oracle.siso_est11n, "mimo_est11n": oracle.mimo_est11n}
    return {"demap": kernels.demap, "deinterleave": graph.deinterleave11a, "demap11n": graph.demap11n, "sig_demap11n": graph.sig_demap11n,
            "siso_est11n": graph.siso_est11n, "mimo_est11n": graph.mimo_est11n}


def recorded_track_frames(fr):
    return [f for f in range(len(fr["nsym"])) if int(fr["nsym"][f]) in REC_TRACK_NSYM]


def recorded_vectors(oracle, e, fn):
    """what engine `e` and the functions `fn` make of the recorded subset of every family -> {name: array}.  The inputs come from `oracle` in both uses (the
    transmitter's L-LTF, the frame's equalised symbols); the contexts of the symbol front end are the LTS family's records as `e` produced them."""
    v = {"seeds": SEEDS}
    _, x = lts_cases(oracle)
    v["lts_rec"], v["lts_post"] = run_lts(e, x)
    sx = symfront_symbols()[:REC_SYM_ROWS]; cr = np.concatenate([v["lts_rec"], random_ctx_records()])
    v["sym_eq"] = run_symfront(e, sx, cr, symfront_index(len(symfront_symbols()), len(cr))[:REC_SYM_ROWS])
    fr = track_frames(oracle)
    out, _, _ = run_track(e, fr, recorded_track_frames(fr))
    v["trk_out"] = np.concatenate([out[int(fr["first"][f]):int(fr["first"][f] + fr["nsym"][f])] for f in recorded_track_frames(fr)])
    v["trk_end"] = run_track(e, fr)[2]
    dx = demap_symbols()[:REC_ROWS]
    for nb in (1, 2, 4, 6):
        v["demap_%d" % nb] = np.stack([fn["demap"](nb, s) for s in dx])
        v["deint_%d" % nb] = np.stack([fn["deinterleave"](nb, s) for s in deint_bytes(nb)[:4]])
        v["demap11n_%d" % nb] = np.stack([fn["demap11n"](nb, s) for s in demap11n_symbols()[:REC_ROWS]])
    v["sig_demap11n"] = np.stack([fn["sig_demap11n"](s) for s in sig_demap11n_symbols()[:REC_ROWS]])
    v["siso_ch"] = np.stack([fn["siso_est11n"](a, b) for a, b in zip(*siso_est11n_lltfs())])
    hh = [fn["mimo_est11n"](a, b) for a, b in zip(*mimo_est11n_ltfs())]
    v["mimo_h"] = np.stack([h for h, _ in hh]); v["mimo_hinv"] = np.stack([hi for _, hi in hh])
    return v
