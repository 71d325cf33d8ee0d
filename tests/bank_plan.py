"""Seeded plans of live changes for the per-receiver down-converter bank, and the model of what every step must leave behind.

A PLAN is a list of steps drawn from a seed by draw() -- never written by hand -- over one fixed frame: 5 receivers on 2 antenna rows, 48 channel
taps per receiver (I and Q filters of different bandwidths, so that a swapped pair shows), NCO steps off the 128 grid, input uniform in
+-30000, 10 to 14 steps of which at least 6 are calls.  str(plan) prints one line per step and Plan.parse() reads it back: a failure message
is its own reproduction, and plan.without(i) is the shrinking step (every step carries the number its arrays are drawn from, and whether a step
is refused is decided by the model from the state it meets, so a plan stays a plan when steps are deleted).

BankModel computes what every step must leave behind.  It is composed of the oracle's stages and of the models the suite already pins to
the oracle (Bank, agc_model, spectrum_model, prefilter_model's tap designs), and every rule is include/msdr.h's, quoted beside the line that
implements it.  Its structure is the header's:
  * per receiver the mixed stream since the last history clear is APPEND-ONLY: every sample is mixed with the oscillator of its own time, an
    antenna switch changes what is appended and not what is there;
  * a call's accumulators are the CURRENT prefilter and channel taps over that stream, taken at D - 1 :: D of the call;
  * everything behind the accumulators is a recurrence with carried state, fed the call's pairs: gain, demodulator, PLL, LMS, nodes, the AGC
    step, the spectrum's tail and cadence;
  * init_fir and reset clear and keep exactly what the header says.
BankModel(plan, orc=None) is the host state machine alone (what is on, what is refused): the generator and the coverage tests run on it.

The oscillator rows are agc_model.nco_rows': the LIBRARY's host-side msdr_nco_q15 (held to a numpy restatement of the header's formulas by
tests/test_nco_host.py), not the oracle's -- so model and CPU tests need the library built, though no GPU.

No GPU code here: tests/test_bank_plan_cases.py holds table and model on the CPU, tests/test_gpu_bank_plans*.py hold the library to the model."""
import ast
import ctypes as C

import numpy as np

import agc_model
import orclib
import prefilter_model
import spectrum_model

CH, ROWS, NT = 5, 2, 48
B = 128
F = np.float32
IN_SCALE = F(1.0 / 32768.0)
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
OK, ARG, LEN = "ok", "arg", "len"
NOUTS = (8, 16, 24, 40, 64, 96)
D2S = (1, 2, 3, 4, 8)
PITCHES = (48, 72, 104)          # the caller's I/Q rows: above n_out for the calls drawn under it (a multiple of 8); 48 and 72 leave calls to refuse
BWS = tuple(1800.0 + 200.0 * k for k in range(17))          # channel bandwidths (bw_taps): 1.8 .. 5 kHz
GAINS = (0.5, 0.75, 1.0, 1.5, 2.0)
SECTIONS = np.array([[0.2066, 0.4131, 0.2066, 0.3695, -0.1958], [0.9766, -1.3815, 0.9766, 1.3815, -0.9533]], F)          # the reference's LP + notch
TABLE_SEED = 20261
# the bank's twelve switches ("Plans of live changes"), by the name of the step that turns each on
SWITCHES = ("retune", "rows", "decim", "prefilter", "meter", "iq", "cx", "gain", "bank_post", "spectrum", "taps", "nodecoef")
GATED = ("prefilter", "cx", "bank_post")          # accepted over a clear FIR history only
EXCLUDED = {frozenset(("prefilter", "cx"))}       # "complex input on (msdr_chain_set_complex_input(on) while a prefilter is set is refused too)"
KINDS = ("call", "retune", "taps", "mode", "nodecoef", "rows", "decim", "meter", "iq", "gain", "gainch", "agc", "spectrum", "anr", "init_fir",
         "reset", "prefilter", "cx", "bank_post")
F32_KINDS = ("call", "retune", "taps", "mode", "rows", "decim", "meter", "iq", "gain", "gainch", "spectrum", "init_fir", "reset", "prefilter", "cx")

_ORC = []


def oracle():
    if not _ORC:
        _ORC.append(orclib.Oracle())
    return _ORC[0]


_TAPS = {}


def bw_taps(bw):
    """test_gpu_osc_per_channel.bw_taps at 48 taps: calc_FIR_coeffs(48, bw), int16"""
    if bw not in _TAPS:
        _TAPS[bw] = np.asarray(oracle().calc_fir_coeffs(NT, float(bw), 70.0, 0, 0.0, 24000.0)[:NT], np.int16).copy()
    return _TAPS[bw]


def off_grid_steps(rng, n):
    """test_gpu_nco_per_channel.off_grid_steps"""
    return rng.integers(1, 1 << 32, n, dtype=np.uint64) | np.uint64(1)


class Bank:
    """test_gpu_nco_per_channel.Bank (the phase of the NEXT sample and the step per channel), with the oscillator rows from agc_model.nco_rows:
    the library's host-side msdr_nco_q15.  tests/test_bank_plan_cases.py holds the two classes to each other."""
    M32 = np.uint64(0xFFFFFFFF)

    def __init__(self, steps, phases):
        self.step, self.phi = np.asarray(steps, np.uint64).copy(), np.asarray(phases, np.uint64).copy()

    def retune(self, first, steps, phases=None):
        steps = np.asarray(steps, np.uint64)
        self.step[first:first + steps.size] = steps
        if phases is not None:
            self.phi[first:first + steps.size] = np.asarray(phases, np.uint64)

    def advance(self, n):
        s, c = agc_model.nco_rows(self.step, self.phi, n)
        self.phi = (self.phi + np.uint64(n) * self.step) & self.M32
        return s, c

    def reset(self):
        self.phi[:] = 0


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
class Plan:
    """seed + frame (f32, pll, post, nodes, sections) + steps; a step is a tuple (kind, uid, parameters ...) of ints"""

    def __init__(self, seed, steps, f32=False, pll=False, post=False, nodes=False, sections=0):
        self.seed, self.steps = int(seed), [tuple(s) for s in steps]
        self.f32, self.pll, self.post, self.nodes, self.sections = bool(f32), bool(pll), bool(post or pll), bool(nodes), int(sections)

    def frame(self):
        return dict(f32=self.f32, pll=self.pll, post=self.post, nodes=self.nodes, sections=self.sections)

    def without(self, i):
        """the shrinking step: the same plan with step i deleted"""
        return Plan(self.seed, self.steps[:i] + self.steps[i + 1:], **self.frame())

    def __str__(self):
        head = "plan seed=%d f32=%d pll=%d post=%d nodes=%d sections=%d" % (self.seed, self.f32, self.pll, self.post, self.nodes, self.sections)
        return "\n".join([head] + ["  %s %s" % (s[0], " ".join(repr(v).replace(" ", "") for v in s[1:])) for s in self.steps])

    @staticmethod
    def parse(text):
        lines = [ln.split() for ln in text.strip().splitlines()]
        kw = {k: int(v) for k, v in (w.split("=") for w in lines[0][1:])}
        seed = kw.pop("seed")
        return Plan(seed, [(ln[0],) + tuple(ast.literal_eval(w) for w in ln[1:]) for ln in lines[1:]], **kw)          # (ints, None and tuples of ints)

    # -- what the frame and the steps are made of: every array from (table seed, plan seed, the step's own number) --
    def rng(self, uid, salt=0):
        return np.random.default_rng([TABLE_SEED, self.seed, int(uid), salt])

    def initial(self):
        """the frame: modes, per-receiver taps, NCO steps and phases, the antenna map -- and the shared tap set the chain is created with"""
        r = self.rng(0, 1)
        pool = (AM, LSB, USB, CW, SYNCAM) if self.pll else (AM, LSB, USB, CW)
        modes = np.array([pool[(c + self.seed) % len(pool)] for c in range(CH)], np.int32)
        ti, tq = self.taps(r, CH)
        return dict(modes=modes, ti=ti, tq=tq, shared_i=self.cast(bw_taps(BWS[3])), shared_q=self.cast(bw_taps(BWS[9])), steps=off_grid_steps(r, CH),
                    phases=r.integers(0, 1 << 32, CH, dtype=np.uint64), rows=np.array([(c + self.seed) % ROWS for c in range(CH)], np.int64))

    def cast(self, t):
        """Q15 taps as they are; fp32 chains get the same filters as floats, t / 32768"""
        return (np.asarray(t, np.float64) / 32768.0).astype(F) if self.f32 else np.asarray(t, np.int16)

    def taps(self, r, count):
        bi, bq = r.integers(0, len(BWS), count), r.integers(0, len(BWS), count)
        bq = np.where(bq == bi, (bq + 5) % len(BWS), bq)          # the I and the Q filter of a receiver differ
        return np.stack([self.cast(bw_taps(BWS[k])) for k in bi]), np.stack([self.cast(bw_taps(BWS[k])) for k in bq])

    def node_rows(self, uid, count):
        r = self.rng(uid)
        return np.stack([oracle().biquad_design(orclib.BQ_NOTCH, float(f), 8.0) for f in r.uniform(600.0, 5000.0, count)]).astype(np.int32)

    def first_nodes(self):
        """the two one-stage nodes the chain is created with: a low-pass and a notch"""
        return [oracle().biquad_design(orclib.BQ_LOWPASS, 5400.0, 0.54), oracle().biquad_design(orclib.BQ_NOTCH, 3000.0, 8.0)]

    def prefilter_row(self, D1, nt):
        return prefilter_model.lowpass(D1, nt, F if self.f32 else np.int16)

    def input(self, uid, n, cx):
        return self.rng(uid, 7).integers(-30000, 30001, (ROWS, n, 2) if cx else (ROWS, n)).astype(np.int16)


# ---- the model --------------------------------------------------------------------------------------------------------------------------------------
class Out:
    """what one call leaves behind (attributes); `status` alone for every other step"""

    def __init__(self, status, **kw):
        self.status = status
        self.__dict__.update(kw)


class BankModel:
    def __init__(self, plan, orc=None, truth=False, mutant=0):
        """orc None: the host state machine alone.  truth (fp32 plans): a float64 twin of every stream beside the fp32 one.  mutant 7: the host rules
        of the library's lib_mut7 build (msdr_chain_reset leaves the spectrum's cadence counter as it was), for survey() to say which plans see it"""
        self.plan, self.orc, self.f32, self.truth, self.mutant = plan, orc, plan.f32, truth and plan.f32, mutant
        ini = plan.initial()
        self.modes, self.ti, self.tq = ini["modes"].copy(), ini["ti"].copy(), ini["tq"].copy()
        self.shared_i, self.shared_q = ini["shared_i"], ini["shared_q"]
        self.bank = Bank(ini["steps"], ini["phases"])
        self.rows = ini["rows"].copy()
        self.D1, self.pre, self.D2, self.cx, self.dir = 1, None, 1, False, 0
        self.meter, self.iq, self.pitch, self.gain_on, self.agc_made = False, False, 0, False, False
        self.rx = [agc_model.Rx(self.f32) for _ in range(CH)]
        self.spec = None          # (bins, power) while the spectrum is on
        self.tick, self.tail = spectrum_model.Tick(1), spectrum_model.Tail(CH, F if self.f32 else np.int16)
        self.anr = np.zeros(CH, np.int32)
        self.clear, self.T = True, 0          # the FIR history is clear; samples since the last clear
        self.on_order = []                    # the switches in the order they were last turned on (coverage)
        self.events = []                      # (T, kind) of the accepted retunes since the last clear, a call between them: generations
        self._retuned = False
        self.pre_entry = plan.post            # until the first step that is not a reset / init_fir in front of msdr_chain_set_bank_post
        if orc is not None:
            self._clear_streams()
            self.pll_st = [orc.syncam_new() for _ in range(CH)]
            self.anr_st = [orc.anr_new() for _ in range(CH)]
            self.node_st = [[orc.biquad_teensy_new([co]) for co in plan.first_nodes()] for _ in range(CH)] if plan.nodes else []
            self._cascade_new()

    # -- helpers --
    def div(self):
        return self.D1 * self.D2

    def np2(self):
        return prefilter_model.pad(NT, self.f32)

    def np1(self):
        return prefilter_model.pad(len(self.pre), self.f32) if self.pre is not None else 0

    def hist_len(self):
        """"the chain keeps raw IF history only, (np2 - 1) * D1 + np1 - 1 samples of it"; one stage: np2 - 1"""
        return prefilter_model.hist_len(self.np1(), self.D1, self.np2()) if self.pre is not None else self.np2() - 1

    def kernel(self):
        """"kernel begins chain_q15pcn2_kernel / chain_f32pcn2_kernel" (prefilter), "chain_q15pcnd_kernel / chain_f32pcnd_kernel" (D > 1), else pcn"""
        return "chain_%spcn%s_kernel" % ("f32" if self.f32 else "q15", "2" if self.pre is not None else "d" if self.D2 > 1 else "")

    def in_force(self):
        """the switches in force for the next call"""
        s = {k for k in ("retune", "rows", "taps", "nodecoef") if k in self.on_order}
        s |= {k for k, v in (("decim", self.D2 > 1), ("prefilter", self.pre is not None), ("meter", self.meter), ("iq", self.iq), ("cx", self.cx),
                            ("gain", self.gain_on), ("bank_post", self.plan.post), ("spectrum", self.spec is not None)) if v}
        return s

    def generations(self):
        """the oscillator generations alive in the window of the next call: the bank of the samples at the window's start, T - hist_len, and every
        retune (two with no call between them count once) that took effect behind it"""
        lo = self.T - self.hist_len()
        return 1 + sum(1 for t in self.events if t > lo)

    def n_samples(self, s):
        """a call's length follows the state it meets: n_out x D1 x D2 (one more where the step is the refusal of a length that is no multiple)"""
        _, _, n_out, _, how = s
        return n_out * self.div() + (1 if how == "len" else 0)

    def _on(self, kind):
        if kind in self.on_order:
            self.on_order.remove(kind)
        self.on_order.append(kind)

    def _off(self, kind):
        if kind in self.on_order:
            self.on_order.remove(kind)

    def _lms_or_pll_at_the_full_rate(self):
        """"Also refused: a Q15 chain created with MSDR_CHAIN_SYNCAM_PLL, a Q15 chain with an LMS channel on ..., all three unless
        msdr_chain_set_bank_post is on" (fp32 chains in this mode have neither)"""
        return not self.f32 and not self.plan.post and (self.plan.pll or bool(self.anr.any()))

    # -- the rules: OK / ARG / LEN of a step in the state it meets --
    def status_of(self, s):
        k = s[0]
        if k == "call":
            audio, n = s[3], self.n_samples(s)
            if not audio and not self.iq:          # "while a buffer is set msdr_chain_process(chain, d_if, NULL, n) is accepted (without one NULL stays refused)"
                return ARG
            if self.plan.nodes and n & 1:          # "Q15 arithmetic needs n_samples even when biquad nodes are present"
                return LEN
            if n % self.div():                     # "n_samples % (D1 * D2) != 0 is MSDR_STATUS_LENGTH_ERROR, nothing enqueued, no state moved"
                return LEN
            n_out = n // self.div()
            if self.plan.nodes and n_out & 1:      # "a Q15 chain with biquad nodes needs n_samples / D even, same error"
                return LEN
            if self.iq and n_out > self.pitch:     # "n_out > pitch is MSDR_STATUS_LENGTH_ERROR: nothing enqueued, no state moved"
                return LEN
            return OK
        if k == "decim":
            D = s[2]
            if D == 0 or D > (59 if self.f32 else 60):          # "Values: 1 .. MSDR_MAX_DECIMATION_Q15 (60) / MSDR_MAX_DECIMATION_F32 (59)"
                return ARG
            if self.pre is not None and not prefilter_model.fits(self.f32, self.np1(), self.D1, self.np2(), D):          # "msdr_chain_set_decimation checks the same rule while a prefilter is set"
                return ARG
            if D > 1 and self._lms_or_pll_at_the_full_rate():
                return ARG
            return OK
        if k == "prefilter":
            D1, nt = s[2], s[3]
            off = D1 == 1 or nt == 0          # "turned off (D1 == 1 or num_taps == 0)"
            if off and self.pre is None:
                return OK
            if not self.clear:                # "set, changed or turned off ... only over a CLEAR FIR history ...; at any other time ARGUMENT_ERROR, nothing changed"
                return ARG
            if off:
                return OK
            if self.cx:                       # "ARGUMENT_ERROR, nothing changed: ... complex input on"
                return ARG
            if self._lms_or_pll_at_the_full_rate():
                return ARG
            return OK if prefilter_model.fits(self.f32, prefilter_model.pad(nt, self.f32), D1, self.np2(), self.D2) else ARG
        if k == "cx":
            on, d = bool(s[2]), s[3] if s[2] else 0
            if on == self.cx and d == self.dir:          # "A repeat call with the values in force does nothing and is always accepted"
                return OK
            if on and self.pre is not None:              # "msdr_chain_set_complex_input(on) while a prefilter is set is refused too"
                return ARG
            return OK if self.clear else ARG             # "the switch, on or off or to the other direction, is accepted only while the FIR history is clear"
        if k == "anr":
            # "a Q15 chain with an LMS channel on (and, while D > 1, msdr_chain_set_anr with any channel on), all three unless msdr_chain_set_bank_post is on"
            return ARG if any(s[2]) and self.div() > 1 and not self.plan.post else OK
        if k == "nodecoef":
            return OK if self.plan.nodes else ARG
        return OK

    # -- a step --
    def apply(self, s):
        st = self.status_of(s)
        if st != OK:          # "nothing changed", "nothing enqueued", "no state moved"
            return Out(st)
        k, uid = s[0], s[1]
        p = self.plan
        if self.pre_entry:          # a plan with the bank's post passes may begin with reset / init_fir in front of msdr_chain_set_bank_post: the chain is not
            if k in ("reset", "init_fir"):          # in phase-accumulator mode yet -- "It changes nothing until the chain is in phase-accumulator mode" -- and the frame's phases come behind it
                return Out(OK)
            self.pre_entry = False
        if k == "call":
            return self._call(s)
        if k == "retune":
            first, count, with_phases = s[2:5]
            r = p.rng(uid)
            steps = off_grid_steps(r, count)
            phases = r.integers(0, 1 << 32, count, dtype=np.uint64) if with_phases else None
            # "The named channels get step[k] from their next sample on.  With phase == NULL the phase carries on ...; otherwise the next sample has phase[k]"
            self.bank.retune(first, steps, phases)
            # "one call is ONE generation for the whole chain, whatever `count`; two calls with no msdr_chain_process between them count once"
            if not self.clear and not self._retuned:
                self.events.append(self.T)
            self._retuned = True
            self._on("retune")
            return Out(OK, args=(first, steps, phases))
        if k == "taps":
            first, count = s[2:4]
            ti, tq = p.taps(p.rng(uid), count)
            self.ti[first:first + count], self.tq[first:first + count] = ti, tq          # "the channel hears the new filter from its next sample on over the old filter's history"
            self._on("taps")
            return Out(OK, args=(first, ti, tq))
        if k == "mode":
            c, m = s[2:4]
            # "msdr_chain_set_mode(chain, ch, mode, tapset) puts channel ch back on shared tap set `tapset` (its own taps are dropped)"
            self.modes[c], self.ti[c], self.tq[c] = m, self.shared_i, self.shared_q
        elif k == "nodecoef":
            node, first, count = s[2:5]
            rows = p.node_rows(uid, count)
            if self.orc is not None:          # "AudioFilterBiquad::setCoefficients(stage, coef) ... history kept"
                for j in range(count):
                    co = np.ascontiguousarray(rows[j], np.int32)
                    self.orc.lib.orc_biquad_teensy_set_coefficients(C.byref(self.node_st[first + j][node]), C.c_uint32(0), co.ctypes.data_as(C.c_void_p))
            self._on("nodecoef")
            return Out(OK, args=(node, first, rows))
        elif k == "rows":
            self.rows = np.array(s[2], np.int64)          # "a live change of the map is an antenna switch: the receiver carries on over its own old history"
            self._on("rows")
        elif k == "decim":
            self.D2 = s[2]          # "A switch of the host's: stream-ordered, may be called at any time, keeps every state"
            (self._on if self.D2 > 1 else self._off)("decim")
        elif k == "prefilter":
            D1, nt = s[2:4]
            if D1 == 1 or nt == 0:
                self.D1, self.pre = 1, None
                self._off("prefilter")
            else:
                self.D1, self.pre = D1, p.prefilter_row(D1, nt)
                self._on("prefilter")
        elif k == "cx":
            self.cx, self.dir = bool(s[2]), (s[3] if s[2] else 0)
            (self._on if self.cx else self._off)("cx")
        elif k == "meter":
            self.meter = bool(s[2])
            (self._on if self.meter else self._off)("meter")
        elif k == "iq":
            self.iq, self.pitch = bool(s[2]), (s[2] or 0)
            (self._on if self.iq else self._off)("iq")
        elif k == "gain":
            # "msdr_chain_set_gain(on): off (default) runs the kernels of a chain without gain and leaves the state alone; on runs the gain twins"
            self.gain_on = bool(s[2])
            self.agc_made = self.agc_made or self.gain_on          # "The state of a receiver is made by the first of these three calls"
            (self._on if self.gain_on else self._off)("gain")
        elif k == "gainch":
            first, count = s[2:4]
            gains = np.array([GAINS[j] for j in p.rng(uid).integers(0, len(GAINS), count)], F)
            for j in range(count):          # "AGC_val = gain[k] ... and its multiplier ... in force from the next call; the ring is untouched"
                self.rx[first + j].set_gain(gains[j])
            self.agc_made = True
            return Out(OK, args=(first, gains))
        elif k == "agc":
            for c in range(CH):             # "0 = held, 1 = stepped"
                self.rx[c].on = int(s[2][c])
            self.agc_made = True
        elif k == "spectrum":
            bins, power, every = s[2:5]
            if not bins and not power:      # "both NULL: off"
                self.spec = None
                self._off("spectrum")
            else:
                if self.spec is None:       # "Off -> on clears tail, counter and count"
                    self.tail.clear()
                    self.tick = spectrum_model.Tick(every)
                    self._on("spectrum")
                # "a call while on with other pointers or another `every` keeps all three (the new `every` loads at the next reload)"
                self.tick.every = every
                self.spec = (bool(bins), bool(power))
        elif k == "anr":
            self.anr = np.array(s[2], np.int32)
        elif k == "init_fir":
            # "zeroes the FIR state and nothing else -- biquad / PLL / LMS state and the mixer's table position persist"; "msdr_chain_init_fir keeps
            # phases and steps"; spectrum: "msdr_chain_init_fir keeps both"
            self._clear_streams()
        elif k == "reset":
            # "FIR state, fp32 cascade state, PLL and LMS state cleared, mixer phase 0.  The Teensy biquad NODES of a Q15 chain keep their history";
            # "msdr_chain_reset sets the chain's time and every phase to 0, keeps the steps and drops the pending generations";
            # "msdr_chain_reset clears tail and counter"; the gain records "live until msdr_chain_destroy"
            self._clear_streams()
            self.bank.reset()
            self.tail.clear()
            if self.mutant != 7:
                self.tick.counter = 0
            if self.orc is not None:
                self.pll_st = [self.orc.syncam_new() for _ in range(CH)]
                self.anr_st = [self.orc.anr_new() for _ in range(CH)]
                self._cascade_new()
        elif k == "bank_post":
            pass          # (the frame's: made before the first msdr_chain_set_nco_channels, "it holds for the rest of the chain's life")
        return Out(OK)

    def _clear_streams(self):
        self.clear, self.T, self.events, self._retuned = True, 0, [], False
        if self.orc is not None:
            dt = F if self.f32 else np.int16
            self.mi = [np.zeros(0, dt) for _ in range(CH)]
            self.mq = [np.zeros(0, dt) for _ in range(CH)]
            if self.truth:
                self.mi64 = [np.zeros(0) for _ in range(CH)]
                self.mq64 = [np.zeros(0) for _ in range(CH)]

    def _cascade_new(self):
        """the fp32 chain's arm_biquad_cascade_df1_f32 per receiver: (instance, its pState) from zero state, and a float64 twin"""
        self.casc = []
        self.casc64 = np.zeros((CH, max(self.plan.sections, 1), 4))
        if self.f32 and self.plan.sections and self.orc is not None:
            self.coefs = np.ascontiguousarray(SECTIONS[:self.plan.sections]).reshape(-1)
            for _ in range(CH):
                S, st = orclib.BiquadDf1(), np.zeros(4 * self.plan.sections, F)
                self.orc.lib.orc_biquad_df1_init_f32(C.byref(S), C.c_uint8(self.plan.sections), self.coefs.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
                self.casc.append((S, st))

    # -- a call --
    def _accumulate(self, c, u_i, u_q, U0, n_out):
        """the current channel pair over the stream u (fs / D1), taken at D2 - 1 :: D2 of the call's part u[U0:]"""
        nt = self.ti.shape[1]

        def window(u):
            lo = U0 - (nt - 1)
            return np.concatenate([np.zeros(max(0, -lo), u.dtype), u[max(0, lo):]])

        if self.f32:
            fi = self.orc.fir_f32_blocks(self.ti[c], window(u_i), B)[nt - 1:][self.D2 - 1::self.D2]
            fq = self.orc.fir_f32_blocks(self.tq[c], window(u_q), B)[nt - 1:][self.D2 - 1::self.D2]
        else:          # agc_model: "an int64 dot product of each mixed stream with pCoeffs in CMSIS order ..., wrapped to int32"
            fi = agc_model.acc_q15(u_i[U0:], self.ti[c], window(u_i)[:nt - 1])[self.D2 - 1::self.D2]
            fq = agc_model.acc_q15(u_q[U0:], self.tq[c], window(u_q)[:nt - 1])[self.D2 - 1::self.D2]
        assert fi.size == n_out and fq.size == n_out
        return fi, fq

    def _call(self, s):
        _, uid, n_out, audio_call, _ = s
        n = self.n_samples(s)
        n_out = n // self.div()
        gens = self.generations()
        out = Out(OK, n=n, n_out=n_out, audio_call=bool(audio_call), kernel=self.kernel(), in_force=self.in_force(), generations=gens,
                  short=n < self.hist_len(), audio=None, pairs=None, meter=None, bins=None, power=None, drew=False)
        if self.orc is None:          # the host state machine alone
            self.bank.phi = (self.bank.phi + np.uint64(n) * self.bank.step) & Bank.M32
            if self.spec is not None:
                out.drew = self.tick.tick()
            self._advance(n)
            return out
        orc = self.orc
        how = s[4]
        if isinstance(how, tuple):          # ("part", first output, outputs of the whole call): a piece of a call that split() cut (the same input)
            x = self.plan.input(uid, how[2] * self.div(), self.cx)[:, how[1] * self.div():how[1] * self.div() + n]
        else:
            x = self.plan.input(uid, n, self.cx)
        out.x = x
        si, sq = self.bank.advance(n)
        audio, pairs, meter = [], [], []
        truth_audio, truth_pairs = [], []
        for c in range(CH):
            row = x[self.rows[c]]          # "receiver c produces, bit for bit, what it would produce if d_if[c] held a copy of row input_row[c]"
            xi, xq = (row[:, 0], row[:, 1]) if self.cx else (row, np.zeros_like(row))
            direction = self.dir if self.cx else 1          # "the chain's real input is its degenerate form: real IF on port 0, zeros on port 1, dir = 1"
            U0 = self.mi[c].size // self.D1
            if self.f32:
                oi, oq = (si[c] / 32768.0).astype(F), (sq[c] / 32768.0).astype(F)          # "F32 x * in_scale * (osc / 32768)"
                mi, mq = orc.freqconv_f32(xi.astype(F) * IN_SCALE, xq.astype(F) * IN_SCALE, oi, oq, direction, 1)
            else:
                mi, mq = orc.freqconv_q15(xi, xq, si[c], sq[c], direction, 1)
            self.mi[c], self.mq[c] = np.concatenate([self.mi[c], mi]), np.concatenate([self.mq[c], mq])
            if self.pre is not None:          # "u[j] = FIR_p over the mixed stream, taken at input sample j * D1 + D1 - 1"
                if self.f32:
                    u_i, u_q = orc.fir_f32_blocks(self.pre, self.mi[c], B)[self.D1 - 1::self.D1], orc.fir_f32_blocks(self.pre, self.mq[c], B)[self.D1 - 1::self.D1]
                else:
                    u_i, u_q = orc.fir_q15_blocks(self.pre, self.mi[c], B)[1][self.D1 - 1::self.D1], orc.fir_q15_blocks(self.pre, self.mq[c], B)[1][self.D1 - 1::self.D1]
            else:
                u_i, u_q = self.mi[c], self.mq[c]
            ai, aq = self._accumulate(c, u_i, u_q, U0, n_out)
            rx = self.rx[c]
            if self.f32:
                # meter: "the two fp32 sums in in_scale units"; gain: "F32 acc * gain, one rounded fp32 multiply, gain = AGC_val after the same clamp"
                pi, pq = ai, aq
                g = agc_model.clamped(rx.val)
                gi, gq = (F(g) * ai, F(g) * aq) if self.gain_on else (ai, aq)
                a = orc.demod_f32(int(self.modes[c]), gi, gq)
                meter.append(float((pi.astype(np.float64) ** 2 + pq.astype(np.float64) ** 2).sum()))
            else:
                # "Q15 ssat16((int64(acc) * multiplier) >> 31)"; "msdr_chain_set_meter keeps measuring the UNGAINED pair"
                pi, pq = agc_model.plain_q15(ai), agc_model.plain_q15(aq)
                gi, gq = (agc_model.pair_q15(ai, rx.mult), agc_model.pair_q15(aq, rx.mult)) if self.gain_on else (pi, pq)
                a = orc.demod_q15(int(self.modes[c]), gi, gq)
                meter.append(int((pi.astype(np.int64) ** 2 + pq.astype(np.int64) ** 2).sum()))
            pairs.append(np.stack([gi, gq], axis=-1))
            if self.truth:
                ta, tp = self._truth(c, xi, xq, si[c], sq[c], direction, U0, n_out, audio_call)
                truth_audio.append(ta)
                truth_pairs.append(tp)
            if audio_call:          # "I/Q-only calls: ... the demodulator and the audio store, the Q15 nodes, the PLL / LMS passes, the fp32 cascade ... do not run and their states are untouched"
                if self.f32:
                    if self.casc:
                        S, _ = self.casc[c]
                        y = np.empty_like(a)
                        orc.lib.orc_biquad_df1_f32_run(C.byref(S), a.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_uint32(a.size))
                        a = y
                else:
                    # "Order: kernel -> PLL -> LMS (anr_kernel) -> biquad nodes, all on n / D samples"; "With gain on the PLL receives the GAINED pair"
                    if self.plan.pll and self.modes[c] == SYNCAM:
                        a = orc.syncam_q15(self.pll_st[c], gi, gq)
                    if self.anr[c]:
                        a = orc.anr_q15(self.anr_st[c], int(self.anr[c]), a)
                    for nd in (self.node_st[c] if self.plan.nodes else ()):
                        a = orc.biquad_teensy_update(nd, a)
                audio.append(a)
            if self.gain_on:          # "behind every successful msdr_chain_process (I/Q-only calls included ...) every receiver whose AGC is on takes ONE step"
                rx.after_call(rx.absmax_of(gi, gq))
        out.pairs, out.audio = np.stack(pairs), (np.stack(audio) if audio_call else None)
        out.meter = np.array(meter, np.float64 if self.f32 else np.uint64)
        if self.truth:
            out.truth_pairs, out.truth_audio = np.stack(truth_pairs), (np.stack(truth_audio) if audio_call else None)
        if self.spec is not None:
            # "the tail becomes the last 64 of (old tail ++ this call's n_out pairs) before anything is drawn"; "gained when gain is on"
            window = self.tail.push(out.pairs)
            out.window = window.copy()
            out.drew = self.tick.tick()
            if out.drew and not self.f32:
                bins = np.stack([spectrum_model.cfft64_q15(orc, w) for w in window])
                out.bins, out.power = bins, np.stack([spectrum_model.power_q15(b) for b in bins])
            elif out.drew:
                z = np.stack([spectrum_model.cfft64_f64(w) for w in window])
                out.bins = np.stack([z.real, z.imag], axis=-1)
                out.power = spectrum_model.display(z.real ** 2 + z.imag ** 2)
        self._advance(n)
        return out

    def _advance(self, n):
        self.T += n
        self.clear, self._retuned = False, False

    def _truth(self, c, xi, xq, si, sq, direction, U0, n_out, audio_call):
        """the same receiver with every operation in float64 (cx_cases.compose_f64 / prefilter_model.model_f64, over the carried stream)"""
        a, b = xi.astype(np.float64) * float(IN_SCALE), xq.astype(np.float64) * float(IN_SCALE)
        s, co = si.astype(np.float64) / 32768.0, sq.astype(np.float64) / 32768.0
        mi, mq = (a * co - b * s, b * co + a * s) if direction else (a * co + b * s, b * co - a * s)
        self.mi64[c], self.mq64[c] = np.concatenate([self.mi64[c], mi]), np.concatenate([self.mq64[c], mq])

        def fir(t, v):
            return np.convolve(v, np.asarray(t, np.float64)[::-1])[:v.size]

        if self.pre is not None:
            u_i, u_q = fir(self.pre, self.mi64[c])[self.D1 - 1::self.D1], fir(self.pre, self.mq64[c])[self.D1 - 1::self.D1]
        else:
            u_i, u_q = self.mi64[c], self.mq64[c]
        fi, fq = fir(self.ti[c], u_i)[U0:][self.D2 - 1::self.D2], fir(self.tq[c], u_q)[U0:][self.D2 - 1::self.D2]
        if self.gain_on:
            g = float(agc_model.clamped(self.rx[c].val))
            fi, fq = g * fi, g * fq
        m = int(self.modes[c])
        y = fi - fq if m == LSB else fi + fq if m == USB else np.sqrt(fi * fi + fq * fq)
        if audio_call and self.plan.sections:
            st = self.casc64[c]
            for k in range(self.plan.sections):          # arm_biquad_cascade_df1_f32's recurrence in float64: y = b0 x + b1 x1 + b2 x2 + a1 y1 + a2 y2
                b0, b1, b2, a1, a2 = (float(v) for v in SECTIONS[k])
                x1, x2, y1, y2 = st[k]
                z = np.empty_like(y)
                for j in range(y.size):
                    v = b0 * y[j] + b1 * x1 + b2 * x2 + a1 * y1 + a2 * y2
                    x2, x1, y2, y1 = x1, y[j], y1, v
                    z[j] = v
                st[k] = (x1, x2, y1, y2)
                y = z
        return y, np.stack([fi, fq], axis=-1)

    # -- what the getters must read after any step --
    def state(self):
        d = dict(nco=[(int(self.bank.step[c]), int(self.bank.phi[c])) for c in range(CH)], decimation=self.D2,
                 prefilter=(self.D1, len(self.pre)) if self.pre is not None else (1, 0), complex_input=(self.cx, self.dir),
                 spectrum=(self.tick.every or 25, self.tick.drawn) if self.spec is not None else None, spectrum_on=self.spec or (False, False),
                 gain=self.gain_on, meter=self.meter, iq=self.pitch if self.iq else 0,
                 agc=[rx.words() for rx in self.rx] if self.agc_made else None)
        if self.orc is not None and self.plan.pll:
            d["pll"] = np.array([[st.fil_out, st.omega2, st.phzerror] for st in self.pll_st], F)
        return d


STATE_KEYS = ("nco", "decimation", "prefilter", "complex_input", "spectrum", "spectrum_on", "gain", "meter", "iq")          # compared with == after every step


def run_model(plan, orc=None, truth=False, mutant=0):
    """-> [(step, Out)] of the whole plan, and the model behind it"""
    m = BankModel(plan, orc, truth, mutant)
    return [(s, m.apply(s)) for s in plan.steps], m


def split(plan):
    """every accepted call of the plan cut in two legal halves (the split-invariance test): -> (plan, the calls' index pairs)"""
    m = BankModel(plan)
    steps, cuts = [], []
    for s in plan.steps:
        if s[0] == "call" and m.status_of(s) == OK:
            q = 2 if plan.nodes else 1
            a = max(q, (s[2] // 2) // q * q)
            steps += [("call", s[1], a, s[3], ("part", 0, s[2])), ("call", s[1], s[2] - a, s[3], ("part", a, s[2]))]
            cuts.append((len(steps) - 2, len(steps) - 1))
            m.apply(s)
        else:
            steps.append(s)
            m.apply(s)
    return Plan(plan.seed, steps, **plan.frame()), cuts


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------------
def frame_of(seed, f32):
    """the frame is the seed's: a quarter of the Q15 plans have the bank's PLL, an eighth the bank's post passes without a PLL, a third nodes; half
    of the fp32 plans run with the reference's two cascade sections"""
    if f32:
        return dict(f32=True, sections=2 if seed % 2 == 0 else 0)
    return dict(pll=seed % 4 == 1, post=seed % 8 == 3, nodes=seed % 3 == 0)


def draw(seed, f32=False):
    """the rule: a plan from its seed"""
    fr = frame_of(seed, f32)
    plan = Plan(seed, [], **fr)
    r = np.random.default_rng([TABLE_SEED, 99, int(f32), seed])
    m = BankModel(plan)
    kinds = F32_KINDS if f32 else KINDS
    n_steps = int(r.integers(10, 15))
    n_calls = int(r.integers(6, n_steps - 2))
    uid = 0
    if plan.post:          # msdr_chain_set_bank_post comes in front of the first msdr_chain_set_nco_channels ("only while the FIR history is clear"): at the
        if n_steps - n_calls >= 4 and r.random() < 0.5:          # plan's start, or behind a reset / init_fir of the chain that is not in the mode yet
            uid += 1
            plan.steps.append((("reset", "init_fir")[int(r.integers(0, 2))], uid))
        uid += 1
        plan.steps.append(("bank_post", uid))
        for s in plan.steps:
            m.apply(s)
    slots = ["x"] * (n_steps - n_calls - len(plan.steps)) + ["call"] * (n_calls - 1)
    r.shuffle(slots)
    slots.append("call")          # a plan ends with a call: whatever the last change was, its effect is compared
    refusal_at = int(r.choice([i for i, k in enumerate(slots) if k == "x"]))
    before = None                 # the kind of the last ACCEPTED step
    for i, slot in enumerate(slots):
        uid += 1
        if slot == "call":
            s = _draw_call(r, m, uid)
        elif i == refusal_at:
            s = _draw_refusal(r, m, uid)
        else:
            s = _draw_change(r, m, uid, kinds, before)
        if m.status_of(s) == OK:
            before = s[0]
        m.apply(s)
        plan.steps.append(s)
    return plan


def _legal_nouts(m):
    return [v for v in NOUTS if not (m.plan.nodes and v & 1) and not (m.iq and v > m.pitch)]


def _draw_call(r, m, uid):
    nouts = _legal_nouts(m)
    short = [v for v in nouts if v * m.div() < m.hist_len()]
    n_out = int(r.choice(short)) if short and r.random() < 0.5 else int(r.choice(nouts))
    audio = 0 if m.iq and r.random() < 0.3 else 1          # "I/Q-only calls: while a buffer is set msdr_chain_process(chain, d_if, NULL, n) is accepted"
    return ("call", uid, n_out, audio, None)


REFUSALS = ("prefilter_history", "prefilter_off_history", "cx_history", "cx_beside_prefilter", "prefilter_beside_cx", "len", "pitch", "odd", "null",
            "decim_range", "decim_fit", "anr_decimated")
RARE = ("prefilter_off_history", "len", "pitch", "odd", "decim_fit", "cx_beside_prefilter", "prefilter_beside_cx", "anr_decimated")          # (drawn four times as often where the state offers them)


def refusal_kind(m, s):
    """which of the header's refusals a refused step is, in the state it meets"""
    k = s[0]
    if k == "call":
        return s[4] if s[4] in ("len", "pitch", "odd", "null") else "call"
    if k == "decim":
        if s[2] == 0 or s[2] > (59 if m.f32 else 60):
            return "decim_range"
        return "decim_fit" if m.pre is not None and not prefilter_model.fits(m.f32, m.np1(), m.D1, m.np2(), s[2]) else "decim"
    if k == "prefilter":
        off = s[2] == 1 or s[3] == 0
        return ("prefilter_off_history" if off else "prefilter_history") if not m.clear else "prefilter_beside_cx" if m.cx else "prefilter"
    if k == "cx":
        return "cx_beside_prefilter" if s[2] and m.pre is not None else "cx_history"
    return "anr_decimated" if k == "anr" else k


def _draw_refusal(r, m, uid):
    """a step that the header refuses in the state it is drawn in"""
    cands = []
    if not m.clear:
        if not m.cx:          # a prefilter set -- or turned off -- over a history that is not clear
            cands.append(("prefilter", uid, 4, 16) if m.pre is None else ("prefilter", uid, 1, 0))
        if m.pre is None:     # the complex-input switch over one
            cands.append(("cx", uid, 0 if m.cx else 1, 0))
    if m.pre is not None:
        cands.append(("cx", uid, 1, 1))                                                                     # complex input beside a prefilter
        misfits = [D for D in range(2, 60) if not prefilter_model.fits(m.f32, m.np1(), m.D1, m.np2(), D)]
        if misfits:           # "msdr_chain_set_decimation checks the same rule while a prefilter is set": a D2 in range whose window does not fit
            cands.append(("decim", uid, int(r.choice(misfits))))
    if m.cx and m.clear:
        cands.append(("prefilter", uid, 2, 16))                                                             # a prefilter beside complex input
    if m.div() > 1:
        cands.append(("call", uid, int(r.choice(_legal_nouts(m))), 1, "len"))                               # a length that is no multiple of D1 x D2
    if m.iq and m.pitch < NOUTS[-1]:
        cands.append(("call", uid, min(v for v in NOUTS if v > m.pitch), 1, "pitch"))                       # n_out above the pitch
    if m.plan.nodes:
        cands.append(("call", uid, int(r.choice((9, 17, 25))), 1, "odd"))                                   # an odd n_out with nodes
    if not m.iq:
        cands.append(("call", uid, 16, 0, "null"))                                                          # an I/Q-only call without a pair buffer
    cands.append(("decim", uid, int(r.choice((0, 61, 1000)))))                                              # a D2 out of range
    if not m.f32 and not m.plan.post and m.div() > 1:
        cands.append(("anr", uid, (0, 1, 0, 2, 0)))                                                         # an LMS channel on a decimating chain without the bank's post passes
    w = np.array([4.0 if refusal_kind(m, s) in RARE else 1.0 for s in cands])
    s = cands[int(r.choice(len(cands), p=w / w.sum()))]
    assert m.status_of(s) != OK, s
    return s


def _draw_change(r, m, uid, kinds, before):
    """an accepted change; over a clear history the history-gated switches are likely, a retune is likely behind a call, a tap change or a
    set_decimation, the LMS filter on a chain that decimates with the bank's post passes, and a stepping AGC where gain is on"""
    for _ in range(200):
        if m.clear and r.random() < 0.6:
            k = ("prefilter", "cx")[int(r.integers(0, 2))]
        elif before in ("call", "taps", "decim") and r.random() < 0.45:
            k = "retune"
        elif "anr" in kinds and m.plan.post and m.div() > 1 and not m.anr.any() and r.random() < 0.3:
            k = "anr"
        elif "agc" in kinds and m.gain_on and not any(rx.on for rx in m.rx) and r.random() < 0.4:
            k = "agc"
        else:
            k = kinds[int(r.integers(1, len(kinds)))]
        first = int(r.integers(0, CH))
        count = int(r.integers(1, CH - first + 1))
        if k == "retune":
            s = (k, uid, first, count, int(r.integers(0, 2)))
        elif k == "taps":
            s = (k, uid, first, count)
        elif k == "mode":
            pool = (AM, LSB, USB, CW, SYNCAM) if m.plan.pll else (AM, LSB, USB, CW)
            s = (k, uid, first, int(pool[int(r.integers(0, len(pool)))]))
        elif k == "nodecoef":
            if not m.plan.nodes:
                continue
            s = (k, uid, int(r.integers(0, 2)), first, count)
        elif k == "rows":
            s = (k, uid, tuple(int(v) for v in r.integers(0, ROWS, CH)))
        elif k == "decim":
            s = (k, uid, int(r.choice([d for d in D2S if d != m.D2])))
        elif k == "meter":
            s = (k, uid, 0 if m.meter else 1)
        elif k == "iq":
            s = (k, uid, 0 if m.iq and r.random() < 0.5 else int(r.choice(PITCHES)))
        elif k == "gain":
            s = (k, uid, 0 if m.gain_on and r.random() < 0.5 else 1)
        elif k == "gainch":
            s = (k, uid, first, count)
        elif k == "agc":
            mask = r.integers(0, 2, CH)
            mask[first] = 1
            s = (k, uid, tuple(int(v) for v in mask))
        elif k == "spectrum":
            if m.spec is not None and r.random() < 0.3:
                s = (k, uid, 0, 0, 0)
            else:
                b, p = ((1, 1), (1, 0), (0, 1))[int(r.integers(0, 3))]
                s = (k, uid, b, p, int(r.integers(1, 4)))
        elif k == "anr":
            if not (m.plan.post or m.div() == 1) or m.f32:
                continue
            s = (k, uid, tuple(int(v) for v in r.integers(0, 3, CH)))
        elif k in ("init_fir", "reset"):
            s = (k, uid)
        elif k == "prefilter":
            if not m.clear:
                continue
            s = (k, uid, 1, 0) if m.pre is not None and r.random() < 0.5 else (k, uid, int(r.choice((2, 4, 8))), int(r.choice((16, 32))))
        elif k == "cx":
            if not m.clear:
                continue
            s = (k, uid, 0, 0) if m.cx and r.random() < 0.5 else (k, uid, 1, int(r.integers(0, 2)))
        else:
            continue
        if m.status_of(s) == OK and not (k in ("prefilter", "cx") and _noop(m, s)):
            return s
    raise AssertionError("no legal change found")


def _noop(m, s):
    return (s[0] == "prefilter" and (s[2] == 1 or s[3] == 0) and m.pre is None) or (s[0] == "cx" and bool(s[2]) == m.cx and (s[3] if s[2] else 0) == m.dir)


# ---- what a plan contributes to the table's coverage conditions (the host state machine alone) ------------------------------------------------------------
def survey(plan):
    """dict: kinds (accepted steps by kind; I/Q-only calls as "call_iq"), refusal_kinds, pairs (the switches in force together in an audio call),
    orders ((a, b): the live switch a was turned on before b, both in force in an audio call), gated_on ((switch, "start" / "init_fir" / "reset"):
    what cleared the history it was turned on over), gated_off, and the counts the conditions name.  "Behind" a step means behind an ACCEPTED
    step: a refused one changed nothing."""
    m = BankModel(plan)
    d = dict(kinds={}, refusal_kinds={}, pairs=set(), orders=set(), gated_on=set(), gated_off=set(), steps=len(plan.steps), calls=0, short=0, gen3=0,
             max_gen=0, retune_behind=0, double_retune=0, refusals=0, iq_only=0, phaseless=0, reset_mid_cadence=0, lms_decimated=0, agc_stepping=0)
    # a reset that moves the cadence where a call can see it: the calls that draw, with and without the counter cleared
    d["reset_mid_cadence"] = int([o.drew for s, o in run_model(plan)[0] if s[0] == "call" and o.status == OK]
                                 != [o.drew for s, o in run_model(plan, mutant=7)[0] if s[0] == "call" and o.status == OK])
    prev, cleared_by = None, "start"
    for s in plan.steps:
        k, st = s[0], m.status_of(s)
        pending = any(t > m.T - m.hist_len() for t in m.events)
        if st != OK:
            d["refusals"] += 1
            name = refusal_kind(m, s)
            d["refusal_kinds"][name] = d["refusal_kinds"].get(name, 0) + 1
        else:
            name = "call_iq" if k == "call" and not s[3] else k
            d["kinds"][name] = d["kinds"].get(name, 0) + 1
            if k == "retune":
                d["retune_behind"] += prev in ("decim", "taps") and pending
                d["double_retune"] += prev == "retune"
                d["phaseless"] += not s[4]
            if k == "bank_post":
                d["gated_on"].add((k, cleared_by))
            if k in ("prefilter", "cx") and not _noop(m, s):
                on = (k == "prefilter" and s[2] > 1 and s[3] > 0) or (k == "cx" and s[2])
                if on:
                    d["gated_on"].add((k, cleared_by))
                else:
                    d["gated_off"].add(k)
            if k == "call":
                d["lms_decimated"] += bool(s[3] and m.anr.any() and m.div() > 1)          # the LMS filter behind the kernel at fs / D (msdr_chain_set_bank_post)
                d["agc_stepping"] += bool(m.gain_on and any(rx.on for rx in m.rx))      # a call behind which AGC() steps a receiver
        out = m.apply(s)
        if st == OK:
            if k == "call":
                cleared_by = None
                d["calls"] += 1
                d["short"] += out.short
                d["gen3"] += out.generations >= 3
                d["max_gen"] = max(d["max_gen"], out.generations)
                d["iq_only"] += not out.audio_call
                if out.audio_call:
                    f = sorted(out.in_force)
                    d["pairs"] |= {frozenset((a, b)) for i, a in enumerate(f) for b in f[i + 1:]}
                    live = [x for x in m.on_order if x in out.in_force and x not in GATED]
                    d["orders"] |= {(a, b) for i, a in enumerate(live) for b in live[i + 1:]}
            elif k in ("init_fir", "reset"):
                cleared_by = k
            prev = k
    return d


def wanted_pairs():
    return {frozenset((a, b)) for i, a in enumerate(SWITCHES) for b in SWITCHES[i + 1:]} - EXCLUDED


def wanted_orders():
    live = [x for x in SWITCHES if x not in GATED]
    return {(a, b) for a in live for b in live if a != b}


# every history-gated switch goes on behind an init_fir and behind a reset (msdr_chain_set_bank_post: in front of the first msdr_chain_set_nco_channels,
# and never off -- "0 after 1 is MSDR_STATUS_ARGUMENT_ERROR")
WANTED_GATED_ON = {(k, by) for k in GATED for by in ("init_fir", "reset")}
WANTED_GATED_OFF = ("prefilter", "cx")
# the counts tests/test_bank_plan_cases.py asserts over the tables and tools/bank_plan_seeds.py chooses the seeds for (reset_mid_cadence, lms_decimated
# and agc_stepping over the Q15 table); a plan has at most 14 steps, so the AGC's ring of 25 wraps in the 30-call CPU trajectory only
WANTED_COUNTS = dict(gen3=6, retune_behind=4, double_retune=1, iq_only=4, reset_mid_cadence=2, lms_decimated=4, agc_stepping=12)
WANTED_REFUSALS = {k: (3 if k in ("len", "pitch", "odd") else 1) for k in REFUSALS}
CANDIDATES = 8000          # tools/bank_plan_seeds.py's default: the seeds below are its output over candidates 0 .. 7999


# ---- the table: the seeds are chosen (tools/bank_plan_seeds.py) so that tests/test_bank_plan_cases.py's coverage conditions hold ---------------------
SEEDS_Q15 = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 120, 214, 286, 518, 533, 746, 997, 1306, 1923, 2625, 3088, 3558, 3663, 3821, 4995, 5751, 5838, 5853)
SEEDS_F32 = (604, 1005, 1049, 1691, 2068, 2756, 4394, 4715, 6145, 6622)


def plans_q15():
    return [draw(s) for s in SEEDS_Q15]


def plans_f32():
    return [draw(s, True) for s in SEEDS_F32]
