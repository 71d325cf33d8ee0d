"""The device's side of a plan (tests/bank_plan.py): a chain of the plan's frame, every step applied through the Python binding, every buffer a
call may write carrying sentinels -- a guard row in front and behind, slack behind n_out -- as test_gpu_decim_per_channel.guarded_call does.
Shared by tests/test_gpu_bank_plans.py (Q15) and tests/test_gpu_bank_plans_f32.py; not collected by pytest."""
import numpy as np

import bank_plan as P
from gpuhelp import msdr

S16, S32 = 0x5A5B, 0x7B5A5B5C
STATUS = {msdr.STATUS_ARGUMENT_ERROR: P.ARG, msdr.STATUS_LENGTH_ERROR: P.LEN}


def fill(n, dtype):
    """n elements of `dtype` whose every 16-bit (32-bit, 64-bit) word is the sentinel"""
    dt = np.dtype(dtype)
    if dt.itemsize == 2:
        return np.full(n, S16, np.uint16).view(dt)
    if dt.itemsize == 4:
        return np.full(n, S32, np.uint32).view(dt)
    return np.full(2 * n, S32, np.uint32).view(dt)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def intact(a):
    return bool((raw(a) == (S16 if a.dtype.itemsize == 2 else S32)).all())


class Got:
    def __init__(self, status, **kw):
        self.status = status
        self.__dict__.update(kw)


class Device:
    def __init__(self, ctx, plan):
        self.ctx, self.plan, self.f32 = ctx, plan, plan.f32
        ini = plan.initial()
        self.adt = np.float32 if self.f32 else np.int16          # audio and pair samples
        self.mdt = np.float64 if self.f32 else np.uint64         # the meter's entries
        self.pdt = np.float32 if self.f32 else np.uint32         # the power's entries
        n = np.arange(128)
        oi, oq = np.round(32767 * np.sin(2 * np.pi * 5 * n / 128)).astype(np.int16), np.round(32767 * np.cos(2 * np.pi * 5 * n / 128)).astype(np.int16)
        if self.f32:          # (the tables a chain with the table mixer is created with; nothing reads them once the oscillator is a phase accumulator)
            oi, oq = (oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)
        kw = {}
        if plan.nodes:
            kw["biquad_nodes"] = [[c] for c in plan.first_nodes()]
        if plan.sections:
            kw["biquad_coeffs"] = P.SECTIONS[:plan.sections]
        self.chain = msdr.Chain(ctx, msdr.ARITH_F32 if self.f32 else msdr.ARITH_Q15, P.CH, ini["shared_i"], ini["shared_q"], mixer=msdr.MIXER_NCO,
                                modes=ini["modes"], osc_i=oi, osc_q=oq, flags=msdr.CHAIN_SYNCAM_PLL if plan.pll else 0, **kw)
        self.ini, self.entered, self.post_done = ini, False, False
        self.meter = self.iq = self.bins = self.power = None
        self.pitch = 0

    def close(self):
        self.chain.close()

    def _enter(self):
        """the frame: the bank's post passes where the plan has them, then per-receiver taps, the oscillator bank, the antenna map"""
        if self.entered:
            return
        c, ini = self.chain, self.ini
        if self.plan.post:
            c.set_bank_post(True)
        (c.set_taps_channels_f32 if self.f32 else c.set_taps_channels)(0, ini["ti"], ini["tq"])
        c.set_nco_channels(0, ini["steps"].astype(np.uint32), ini["phases"].astype(np.uint32))
        c.set_input_rows(ini["rows"], P.ROWS)
        self.entered = True

    def apply(self, s, want, n=None, cx=False):
        """one step; `want` is the model's Out of it (the arrays a setter takes are the model's), n / cx the length and input kind of a call"""
        if s[0] == "bank_post":
            self.chain.set_bank_post(True)
            self.post_done = True
            return Got(P.OK)
        if self.plan.post and not self.entered and not self.post_done and s[0] in ("reset", "init_fir"):
            # in front of msdr_chain_set_bank_post, on the chain that is not in phase-accumulator mode yet: the switch goes on over the history this cleared
            (self.chain.reset if s[0] == "reset" else self.chain.init_fir)()
            return Got(P.OK)
        self._enter()
        try:
            if s[0] == "call":
                return self._call(s, n, cx)
            self._set(s, want)
        except msdr.MsdrError as e:
            return Got(STATUS[e.status], text=str(e))
        return Got(P.OK)

    def _set(self, s, want):
        c, k = self.chain, s[0]
        if k == "retune":
            first, steps, phases = want.args if want.status == P.OK else (s[2], P.off_grid_steps(self.plan.rng(s[1]), s[3]), None)
            c.set_nco_channels(first, steps.astype(np.uint32), None if phases is None else phases.astype(np.uint32))
        elif k == "taps":
            first, ti, tq = want.args
            (c.set_taps_channels_f32 if self.f32 else c.set_taps_channels)(first, ti, tq)
        elif k == "mode":
            c.set_mode(s[2], s[3])
        elif k == "nodecoef":
            rows = want.args[2] if want.status == P.OK else self.plan.node_rows(s[1], s[4])
            c.set_node_coefficients_channels(s[2], s[3], 0, rows)
        elif k == "rows":
            c.set_input_rows(np.array(s[2], np.int64), P.ROWS)
        elif k == "decim":
            c.set_decimation(s[2])
        elif k == "prefilter":
            c.set_prefilter(s[2], None if s[2] == 1 or s[3] == 0 else self.plan.prefilter_row(s[2], s[3]))
        elif k == "cx":
            c.set_complex_input(bool(s[2]), s[3])
        elif k == "meter":
            self.meter = self.ctx.to_device(fill(P.CH + 1, self.mdt)) if s[2] else None
            c.set_meter(self.meter)
        elif k == "iq":
            if s[2]:          # a guard row in front and behind
                buf = self.ctx.to_device(fill((P.CH + 2) * s[2] * 2, self.adt))
                c.set_iq_out(buf.offset(s[2] * 2 * np.dtype(self.adt).itemsize), s[2])
                self.iq, self.pitch = buf, s[2]
            else:
                c.set_iq_out(None)
                self.iq, self.pitch = None, 0
        elif k == "gain":
            c.set_gain(bool(s[2]))
        elif k == "gainch":
            c.set_gain_channels(want.args[0], want.args[1])
        elif k == "agc":
            c.set_agc(np.array(s[2], np.int32))
        elif k == "spectrum":
            bins = self.ctx.to_device(fill((P.CH + 1) * 128, self.adt)) if s[2] else None
            power = self.ctx.to_device(fill((P.CH + 1) * 64, self.pdt)) if s[3] else None
            c.set_spectrum(bins, power, s[4])
            self.bins, self.power = bins, power
        elif k == "anr":
            c.set_anr(np.array(s[2], np.int32))
        elif k == "init_fir":
            c.init_fir()
        elif k == "reset":
            c.reset()
        else:
            raise AssertionError(s)

    def _call(self, s, n, cx):
        ctx, c = self.ctx, self.chain
        audio_call = bool(s[3])
        how = s[4]
        if isinstance(how, tuple):
            raise AssertionError("pieces of a call belong to the model's split test")
        x = self.plan.input(s[1], n, cx)
        div = max(1, c.decimation() * c.prefilter()[0])
        n_out = -(-n // div)
        guard = 2 * n_out + 8
        flat = fill(guard + P.CH * n_out + P.CH * 8 + guard, self.adt)
        dy = ctx.to_device(flat)
        for buf, dt in ((self.meter, self.mdt), (self.iq, self.adt), (self.bins, self.adt), (self.power, self.pdt)):
            if buf is not None:          # every buffer a call may write starts as sentinels
                buf.upload(fill(buf.download().size, dt))
        status, text = P.OK, ""
        try:
            c.process(ctx.to_device(np.ascontiguousarray(x)), dy.offset(guard * flat.itemsize) if audio_call else None, n)
        except msdr.MsdrError as e:
            status, text = STATUS[e.status], str(e)
        back = dy.download()
        got = Got(status, text=text, audio=None, pairs=None, meter=None, bins=None, power=None, drew=False, kernel=c.info()["kernel"], flavour=c.info()["flavour"])
        ok = status == P.OK
        body = back[guard:guard + P.CH * n_out]
        got.guards = intact(back[:guard]) and intact(back[guard + P.CH * n_out:]) and (intact(body) if not (ok and audio_call) else True)
        if ok and audio_call:
            got.audio = body.reshape(P.CH, n_out).copy()
        if self.iq is not None:
            pb = self.iq.download().reshape(P.CH + 2, self.pitch, 2)
            got.guards = got.guards and intact(pb[0]) and intact(pb[-1]) and intact(pb[1:-1, n_out:] if ok else pb)
            if ok:
                got.pairs = pb[1:-1, :n_out].copy()
        if self.meter is not None:
            m = self.meter.download()
            got.guards = got.guards and intact(m[P.CH:] if ok else m)
            if ok:
                got.meter = m[:P.CH].copy()
        drew = []
        for name, buf, per in (("bins", self.bins, 128), ("power", self.power, 64)):
            if buf is None:
                continue
            v = buf.download().reshape(P.CH + 1, per)
            got.guards = got.guards and intact(v[P.CH:])          # the guard row behind the last receiver
            drew.append(not intact(v[:P.CH]))
            got.guards = got.guards and (ok or not drew[-1])          # a call that returns an error "moves neither tail nor counter ... and writes nothing"
            if drew[-1]:
                assert not any(intact(row) for row in v[:P.CH]), "a drawing call overwrites all `channels` rows"
                setattr(got, name, v[:P.CH].reshape((P.CH, 64, 2) if per == 128 else (P.CH, 64)).copy())
        assert len(set(drew)) <= 1, "one spectrum buffer was written and the other was not"
        got.drew = bool(drew and drew[0])
        return got

    def state(self):
        """what the getters read: the shape of BankModel.state()"""
        c = self.chain
        if not self.entered:
            return None
        sp = c.spectrum()
        d = dict(nco=[c.nco(ch) for ch in range(P.CH)], decimation=c.decimation(), prefilter=c.prefilter(), complex_input=c.complex_input(),
                 spectrum=(sp[2], sp[3]) if (sp[0] or sp[1]) else None, spectrum_on=(sp[0] is not None, sp[1] is not None), agc=None, gain=c.gain(),
                 meter=c.meter() is not None, iq=int(c.iq_out()[1]) if c.iq_out()[0] is not None else 0)
        try:
            d["agc"] = [c.agc_state(ch)["words"] for ch in range(P.CH)]
        except msdr.MsdrError:          # "this chain has no gain state": none of the three setters was called yet
            pass
        if self.plan.pll:
            d["pll"] = np.stack([c.pll_state(ch) for ch in range(P.CH)])
        return d
