"""Hand-sequenced NVF train / latent / eval steps on the gfx950 kernels.

The reference runs one step as ~1 500 aten ops driven by autograd with ~14 host syncs
(NVFPCC.py:149-250).  Here a step is a fixed list of C-ABI launches on one HIP stream, with

  * every leaf block's grids and the latent table resident in HBM (no DataLoader process),
  * all 28 decoder parameter tensors living in ONE flat buffer (and their gradients in another),
    so Adam is a single fused launch and the data-parallel exchange is a single RCCL all-reduce,
  * all ten layers' effective weights produced by one table-driven launch,
  * the ReLU / sigmoid backward, the head gradients' addition and the loss gradient fused into the
    kernels that produce or consume them,
  * no host synchronisation inside a step (rate coefficients come from per-block point counts
    precomputed on the host).

Result-preserving shortcuts taken from the reference's own data flow: the mini-batch phase never
uses the latent gradients (they are zeroed at NVFPCC.py:226) and the latent phase never uses the
decoder weight gradients (zeroed at NVFPCC.py:150), so each phase skips the half it discards.
"""
import functools
import os
from typing import NamedTuple

import numpy as np
import torch

from . import ops, routes
from ._lib import lib, check, NvfLayerDesc
from .network import NoiseState

R, S, NONE = ops.ACT_RELU, ops.ACT_SIGMOID, ops.ACT_NONE
# winograd=None: the 4^3 layers of a training step in the Winograd (y, x) form (conv_wino.hip, conv16_wino.hip);
# NVF_WINO=0 keeps the direct summation order (the strict-trajectory engine)
_WINO = os.environ.get("NVF_WINO", "1") != "0"


# One-launch groupings of the step.  Plain constants: tests/test_gpu_engine.py switches the first four off to build the
# separate-launch reference its bit-equality tests compare against; bench.py reads _HEADS_IN_TRUNK5.
_HEAD_BIAS_IN_LOSS = True   # heads' bias gradients from the loss launch
_SUMS_IN_TRUNK5 = True      # partial bias sums inside the five-gradient launch
# the stem's backward (conv0^T -> IGDN' -> up0^T, up0's gradients) as the first workgroups of the five-gradient launch
# instead of two launches in front of it (csrc/stem_bwd.h): it needs g1 only and feeds the latent tail only
_STEM_IN_TRUNK5 = True
# the stem's FORWARD (latent generator + quantiser + up0 / IGDN / conv0) inside the step head's launch: its workgroups
# derive their weights from the raw parameters, so the two latency-bound launches have nothing to wait for in each other
_STEM_IN_HEAD = True
_HEADS_IN_TRUNK5 = True     # heads' weight gradients as workgroups of the five-gradient launch (narrow decoder)
# Most blocks one full-batch pass (latent step, evaluation) holds resident: the largest batch these passes have been
# run and measured at (tools/latent4096.py).  A larger shard -- a group of frames -- is walked in chunks of this size.
LATENT_CHUNK = 4096


class StepPlan(NamedTuple):
    """The launches one step consists of (plan_step).  batch_and_prepare, forward and backward branch on these fields only."""
    want_w: bool                # decoder gradients (the mini-batch phase)
    want_emb: bool              # latent gradients (the latent phase)
    stem_fwd: str               # "head": in the step head's launch / "latent": with the latent generator / "fused" / "layers"
    latent_fwd_fused: bool      # latent generator + quantiser in one launch (where the stem's forward did not take them)
    heads: str                  # "deferred": forward too in the loss launch / "fused_loss" / "heads3" / "layers" /
                                # "main": conv2_cls alone, the coarse heads do not run (latent passes under a frozen decoder)
    head_bias_in_loss: bool     # the heads' bias gradients are partials of the loss launch
    heads_in_trunk5: bool       # the heads' weight gradients are workgroups of the five-gradient launch
    trunk5: bool                # the five trunk weight gradients in one launch (add_trunk5); else per layer
    conv0_wgrad_in_stem: bool   # conv0's weight gradient rides in the stem's backward
    stem_bwd: str               # "queued": inside the five-gradient launch / "partial" / "plain" / "layers"
    tail_queued: bool           # the latent tail rides in the next weight-gradient launch; else three launches
    sums_in_trunk5: bool        # partial bias sums inside the five-gradient launch (where the step head carried the rate job)
    fused_optimiser: bool       # Adam + epoch sums inside the slab reduction and the finals launch (single GPU)


@functools.lru_cache(maxsize=None)
def plan_step(narrow, wide, winograd, fused_stem, fused_latent_stem, heads3, ch, batch, want_w, want_emb, fuse, hook,
              naive, head_bias_in_loss, sums_in_trunk5, stem_in_trunk5, stem_in_head, heads_in_trunk5,
              step_head=False, defer_heads=False, main_only=False):
    """Which launches a step of ``batch`` blocks consists of, from the engine's class flags, the caller's request (``fuse``:
    it handed over the optimiser's coefficients; ``step_head``: batch_and_prepare(stem_mode=...) ran; ``defer_heads``:
    forward(defer_heads=True)), ops._NAIVE and the five module switches.  No tensors.  What launch_trunk_wgrads (wgrad.hip)
    answers with NVF_EINVAL is an implication between the fields (tests/test_step_plan.py).  ``winograd`` and the 64-block
    switch point select kernel forms inside a launch (routes.py), never a launch.  ``main_only``: a latent pass whose
    objective holds the main output's focal term alone -- the coarse heads (conv0_cls, conv1_cls) run neither forward, loss
    nor backward-data (a decoder rebuilt from a pack holds seed values there: the pack drops them)."""
    if main_only and want_w:
        raise ValueError("plan_step: main_only is a form of the latent pass (no weight gradients)")
    # the one-launch groupings bypass the variant switch of the per-layer entry points: only with the tuned kernels
    tuned = naive == 0
    small = batch <= 32         # the cooperative launches keep one arrival counter per block, 32 of them
    stem_fwd = ("head" if step_head and stem_in_head and fused_stem and fused_latent_stem and small and tuned else
                "latent" if ch <= 8 and tuned and fused_stem and fused_latent_stem else
                "fused" if fused_stem else "layers")
    fused_loss = heads3 and small and tuned
    heads = ("main" if main_only else ("deferred" if defer_heads and want_w else "fused_loss") if fused_loss else
             "heads3" if heads3 else "layers")
    trunk5 = want_w and narrow and tuned
    in_trunk5 = trunk5 and heads3 and heads_in_trunk5
    tail = want_w and not want_emb and ch <= 8 and tuned
    stem_bwd = ("queued" if stem_in_trunk5 and tail and in_trunk5 and fused_stem and small else
                "layers" if not fused_stem else "partial" if want_w else "plain")
    return StepPlan(want_w=want_w, want_emb=want_emb, stem_fwd=stem_fwd, latent_fwd_fused=ch <= 8 and tuned, heads=heads,
                    head_bias_in_loss=want_w and head_bias_in_loss and fused_loss, heads_in_trunk5=in_trunk5,
                    trunk5=trunk5, conv0_wgrad_in_stem=want_w and fused_stem and not trunk5, stem_bwd=stem_bwd,
                    tail_queued=tail, sums_in_trunk5=in_trunk5 and sums_in_trunk5, fused_optimiser=fuse and not hook)


def _abandons_step(fn):
    """A step entry point of TrainEngine: any exception out of it leaves "no step in flight" behind (_abandon_step).  The
    handler is the only addition to a step that succeeds: no launch, no sync."""
    @functools.wraps(fn)
    def run(self, *args, **kw):
        try:
            return fn(self, *args, **kw)
        except BaseException:
            self._abandon_step()
            raise
    return run


TRUNK = ("up0", "conv0", "up1", "conv1", "up2", "conv2", "conv2_cls")
HEADS = ("conv1_cls", "conv0_cls")

_DESC = np.dtype(NvfLayerDesc)      # a row of the layer table (include/nvf_hip.h)


class _Layer:
    __slots__ = ("name", "mod", "kind", "k", "w_fwd", "w_bwd", "b_eff", "gk", "gb", "cin", "cout", "pad", "wp")


class TrainEngine:
    def __init__(self, net, gt_all, dist_all, n_points_total, lmbda, w1, w2, lr, wemb, emb=None, seed=0, winograd=None):
        assert lib().nvf_layer_desc_size() == _DESC.itemsize
        # winograd=False (or NVF_WINO=0): every 4^3 layer of a training step keeps the direct summation order -- 0.41 ms
        # per step instead of 0.35, and the reference's own three-epoch trajectory reproduced to 1e-7 instead of
        # statistically (tests/test_gpu_engine.py, the trajectory golden)
        self.winograd = _WINO if winograd is None else bool(winograd)
        self.net = net
        self.dev = gt_all.device
        self.gt, self.dist = gt_all.contiguous(), dist_all.contiguous()
        self.N_leaf = self.gt.shape[0]
        self.n_points_total = float(n_points_total)
        self.lmbda, self.w1, self.w2 = float(lmbda), float(w1), float(w2)
        self.lr, self.lr_emb = float(lr), float(lr) * float(wemb)
        self.seed = int(seed)
        # Counter behind both noise sources (weight noise at q = 1, latent rate-proxy noise in every train-mode
        # forward): it advances once per train / latent step WHATEVER q is -- the reference draws a fresh
        # torch.rand_like(x) on every mode='train' forward (network.py:4516), also after --phase_change.  Every rank
        # advances it identically (idle ranks of a short last batch included, NVFPCC.py train()).
        self.noise_step = 0
        self.rate_grad_scale = 1.0   # 1/world_size under data parallelism: the weight-rate term is replicated
        self.grad_hook = None        # called on flat_g between backward and Adam (RCCL all-reduce)
        self.opt_step = 0
        self.emb_step = 0
        self.ch = net.entropy_coder.sigma.shape[1]
        self.channels = net.reconstructor.channels
        # GT pyramid and per-block occupied-voxel counts, once (MultiscaleProcessor, NVFPCC.py:76-88)
        self.gt16 = ops.maxpool2(self.gt)
        self.gt8 = ops.maxpool2(self.gt16)
        self.counts = self.gt.sum(dim=(1, 2, 3, 4)).double().cpu().numpy()
        # latent table + its Adam state (NVFPCC.py:120-124)
        self.emb = (torch.ones(self.N_leaf, self.ch, 2, 2, 2, device=self.dev) if emb is None
                    else emb.detach().to(self.dev).float().contiguous().clone())
        self.emb_m = torch.zeros_like(self.emb)
        self.emb_v = torch.zeros_like(self.emb)
        # Decoder classes ("Decoder configurations"): the two of BASELINE.json have matrix-core / fused
        # launches instantiated for their shapes; ANY other --chanstr runs every layer on the shape-generic kernels
        # (conv3d_gather, convT3d_k5s2_fwd, wgrad_tiled; per-layer stem, heads and gradients) -- same results, not tuned
        chans = tuple(net.reconstructor.channels)
        self.narrow = chans == (8, 16, 8, 8)
        self.wide = chans == (16, 32, 16, 16)
        self.generic = not (self.narrow or self.wide)
        self.decoder_class = "narrow" if self.narrow else "wide" if self.wide else "generic"
        self._flatten_parameters()
        self._build_layers()
        self.last = {}
        # per-step scalars live in device memory while a captured HIP graph replays (see GraphedTrainStep)
        self._step_dev = None     # uint64 noise-step offset
        # every launch of a step goes to the current stream: a two-stream schedule stopped paying once the kernels were
        # fast (round 1, batch 16: 0.828 ms either way -- every kernel fills the chip on its own)
        self.fused_stem = (self.narrow or self.wide) and net.entropy_coder.sigma.shape[1] <= 8   # stem in fused launches
        self.fused_latent_stem = True      # latent generator + quantiser ride in the stem's forward launch
        self._g_lat_dev = None    # lambda * w1 / n_pts
        self._wg = None
        self.ctx = ops.StepCtx()  # deferred final passes + queued latent tail of the step in flight (caller-owned)
        self.ctx.set_direct(not self.winograd)
        self.epoch_acc = None     # float[16] epoch sums written by nvf_step_tail (enable_epoch_stats)
        self._tail_done = torch.zeros(2, dtype=torch.int32, device=self.dev)   # nvf_step_tail's arrival counter
        self._coef_live = torch.zeros(2, device=self.dev)   # the step's Adam coefficients, staged outside the step buffer
        self._rate = None         # (NvfRateJob, {gk data_ptr: its weight-rate gradient}, rate_grad_scale) of the step head
        self._rate_ready = False  # the step head of the step in flight carried the weight-rate partial pass
        self._rate_retired = []   # outgrown weight-rate buffers stay referenced (kernels in flight)
        self._graphs_captured = 0  # GraphedTrainStep instances that baked this engine's buffers into a graph
        self.tail_done = False    # the last backward pass applied the optimiser itself (fused tail)
        self._tail_ranges = {}    # gradient index ranges no fused launch covers, per set of covered intervals
        self.collective_mode = None   # "graph" / "host": where GraphedTrainStep puts the all-reduce (dist.attach)
        # the three classifier heads go through the one-launch kernels (instantiated for the two decoders of BASELINE.json);
        # the one-launch trunk weight gradients exist for the narrow decoder only
        self.heads3 = self.narrow or self.wide

    # ------------------------------------------------------------------ parameters
    def _flatten_parameters(self):
        named = list(self.net.named_parameters())
        total = sum(p.numel() for _, p in named)
        self.flat_p = torch.empty(total, device=self.dev)
        # gradients + 32 floats behind them: [0, 18) = the step's metric counts (ops.metrics3: main output, head 0,
        # head 1).  They ride in the data-parallel all-reduce of the gradients, so the per-step accuracy RATIOS the
        # reference logs (NVFPCC.py:214-221) are those of the whole mini-batch whatever the number of ranks
        self.flat_gx = torch.zeros(total + 32, device=self.dev)
        self.flat_g = self.flat_gx[:total]
        self.step_counts = self.flat_gx[total:total + 18]
        self.flat_m = torch.zeros(total, device=self.dev)
        self.flat_v = torch.zeros(total, device=self.dev)
        self.slices = {}
        off = 0
        for name, p in named:
            n = p.numel()
            self.flat_p[off:off + n].copy_(p.detach().reshape(-1))
            p.data = self.flat_p[off:off + n].view(p.shape)
            p.grad = self.flat_g[off:off + n].view(p.shape)
            self.slices[name] = (off, n)
            off += n

    def _g(self, name):
        off, n = self.slices[name]
        return self.flat_g[off:off + n]

    def _build_layers(self):
        rec = self.net.reconstructor
        mods = [("latent", self.net.latent_gen.h_analysis_2, "latent_gen.h_analysis_2")]
        mods += [(n, getattr(rec, n), "reconstructor." + n) for n in TRUNK + HEADS]
        self.layers = {}
        table = np.zeros(len(mods), _DESC)
        for i, (name, m, prefix) in enumerate(mods):
            L = _Layer()
            L.name, L.mod = name, m
            L.kind = 1 if m.kernel.shape[2] == 5 else 0      # k=5 layers are the transposed convs
            L.k = m.kernel.shape[2]
            n = m.kernel.numel()
            L.w_fwd = torch.empty(n, device=self.dev)
            L.w_bwd = torch.empty(n, device=self.dev)
            L.b_eff = torch.empty(m.b.numel(), device=self.dev)
            L.gk, L.gb = self._g(prefix + ".kernel").view(m.kernel.shape), self._g(prefix + ".b")
            L.cin, L.cout, L.pad = m.in_channels, m.out_channels, m.padding
            # the matrix-core forms' packed weights (routes.PACKS), re-packed after every weight preparation
            L.wp = {p: torch.empty(routes.pack_floats(lib(), p, L.cin, L.cout, L.k), device=self.dev)
                    for p in routes.layer_packs(self.decoder_class, self.winograd, name, L.cin, L.cout, L.k, L.pad)}
            self.layers[name] = L
            t = table[i]
            t["kernel"], t["kernel_init"] = m.kernel.data_ptr(), m.kernel_init.data_ptr()
            t["b"], t["b_init"] = m.b.data_ptr(), m.b_init.data_ptr()
            t["w_fwd"], t["w_bwd"], t["b_eff"] = L.w_fwd.data_ptr(), L.w_bwd.data_ptr(), L.b_eff.data_ptr()
            t["dim0"], t["dim1"], t["k3"] = m.kernel.shape[0], m.kernel.shape[1], L.k ** 3
            t["kind"] = L.kind
            t["quantised"] = 1 if name in TRUNK else 0
            t["layer_id"] = m.layer_id
            t["nbias"] = m.b.numel()
        row = {name: i for i, (name, _, _) in enumerate(mods)}
        self._rows = row
        # packing by packing in routes.PACKS order, layers in table order, is the job order inside nvf_pack_mfma_all /
        # nvf_step_head
        jobs, meta = [], []
        for pack, P in routes.PACKS.items():
            for nm, L in self.layers.items():
                if pack in L.wp:
                    jobs.append((getattr(L, P.src), L.wp[pack]) + routes.pack_job(pack, L.cin, L.cout, L.k))
                    meta.append((row[nm], int(P.src == "w_bwd")))
        assert len(jobs) <= 16
        self._mfma_jobs = jobs
        self._mfma_job_layers = meta           # (layer-table row, 0 = w_fwd / 1 = w_bwd) of each job's source
        self._table_host = table
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(self.dev)
        self.nlayers = len(mods)

    def _rate_job(self):
        """The weight-rate term's partial pass as a job of the step head: it reads parameters only.  g is a host
        constant (lambda w2 / N, times 1 / world under data parallelism)."""
        key = (self.rate_grad_scale, self.lmbda, self.w2, self.n_points_total)
        if self._rate is not None and self._rate[2] != key:
            # captured step graphs hold the old buffers' addresses and the old g: a graph replayed after this point would
            # add stale addends into retired memory -- refuse instead (dist.attach runs before any capture)
            if self._graphs_captured:
                raise RuntimeError("weight-rate coefficients changed after a step graph was captured "
                                   "(attach data parallelism / set lambda before building GraphedTrainStep)")
            self._rate_retired.append(self._rate)       # a kernel in flight may still read them
        if self._rate is None or self._rate[2] != key:
            lm = self.net.reconstructor.likelihood_model
            ks = [self.layers[n].mod.kernel for n in TRUNK]
            dk = torch.zeros(sum(k.numel() for k in ks), device=self.dev)
            dks, off = [], 0
            for k in ks:
                dks.append(dk[off:off + k.numel()])
                off += k.numel()
            part = torch.zeros(3 * 512, device=self.dev)
            g = self.lmbda * self.w2 / self.n_points_total * self.rate_grad_scale
            job = ops.rate_job(ks, dks, lm.sigma, lm.mu, part, g)
            add = {self.layers[n].gk.data_ptr(): d for n, d in zip(TRUNK, dks)}
            self._rate = (job, add, key, dk, part)
        return self._rate

    def _plan(self, batch, want_w=False, want_emb=False, fuse=False, step_head=False, defer_heads=False, main_only=False):
        """plan_step for this engine, with the module switches and ops._NAIVE as they are NOW (tests and bench.py assign them)."""
        return plan_step(self.narrow, self.wide, self.winograd, self.fused_stem, self.fused_latent_stem, self.heads3,
                         self.ch, batch, want_w, want_emb, fuse, self.grad_hook is not None, ops._NAIVE,
                         _HEAD_BIAS_IN_LOSS, _SUMS_IN_TRUNK5, _STEM_IN_TRUNK5, _STEM_IN_HEAD, _HEADS_IN_TRUNK5,
                         step_head, defer_heads, main_only)

    def _noise(self):
        """(step, step_dev) of the counter RNG: the host's counter, or 0 and the device word a captured graph reads."""
        sd = self._step_dev
        return (0 if sd is not None else self.noise_step), sd

    def _ec(self):
        """The entropy coder's (sigma, mu), flattened."""
        ec = self.net.entropy_coder
        return ec.sigma.reshape(-1), ec.mu.reshape(-1)

    def batch_and_prepare(self, idx_dev, q, with_rate=False, stem_mode=None):
        """_batch(idx_dev) and prepare_weights(q) -- row gather, effective weights, MFMA packings -- as ONE launch
        (``with_rate``: + the weight-rate term's partial sums, consumed by the backward pass of the same step).  Returns
        the five gathered tensors (gt, dist, gt16, gt8, e).  ``stem_mode`` = 'train' / 'eval': + the stem's forward of
        this mini-batch in the same launch where the decoder has one (nvf_step_head_stem); a sixth member is then the
        dict of its activations for forward(e, stem_mode, idx_dev, stem=...), or None if the caller's forward() has to
        run the stem itself."""
        import ctypes
        srcs = [self.gt, self.dist, self.gt16, self.gt8, self.emb]
        n, rows = len(srcs), idx_dev.numel()
        dsts = [torch.empty((rows,) + tuple(s.shape[1:]), device=s.device) for s in srcs]
        step, sd = self._noise()
        jobs, meta = self._mfma_jobs, self._mfma_job_layers
        npk = len(jobs)
        iarr = lambda xs: (ctypes.c_int * max(len(xs), 1))(*xs)
        args = (self.table.data_ptr(), self.nlayers, int(q), self.seed, step, None if sd is None else sd.data_ptr(),
                (ctypes.c_void_p * max(npk, 1))(*[j[1].data_ptr() for j in jobs]), iarr([j[2] for j in jobs]),
                iarr([j[3] for j in jobs]), iarr([j[4] for j in jobs]), iarr([m[0] for m in meta]),
                iarr([m[1] for m in meta]), npk, (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs]),
                (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts]), (ctypes.c_int * n)(*[s[0].numel() for s in srcs]), n,
                idx_dev.data_ptr(), rows, ctypes.byref(self._rate_job()[0]) if with_rate else None)
        o = None
        if self._plan(rows, step_head=stem_mode is not None).stem_fwd == "head":
            from ._lib import NvfStemHead
            net = self.net
            g2, ec, ig = net.latent_gen.gdn_2, net.entropy_coder, net.reconstructor.activation
            dev, ch = self.dev, self.ch
            c0, c1 = self.channels[0], self.channels[1]
            o = {"h": torch.empty(rows, ch, 2, 2, 2, device=dev), "lat": torch.empty(rows, ch, 2, 2, 2, device=dev),
                 "x0": torch.empty(rows, ch, 2, 2, 2, device=dev), "lbits": torch.empty(1, device=dev),
                 "a0": torch.empty(rows, c0, 4, 4, 4, device=dev), "h0": torch.empty(rows, c0, 4, 4, 4, device=dev),
                 "y1": torch.empty(rows, c1, 8, 8, 8, device=dev)}
            sj = NvfStemHead()
            sj.emb, sj.lat_beta_hat, sj.lat_gamma_hat = self.emb.data_ptr(), g2.beta.data_ptr(), g2.gamma.data_ptr()
            sj.sigma, sj.mu = ec.sigma.data_ptr(), ec.mu.data_ptr()
            sj.beta_hat, sj.gamma_hat = ig.beta.data_ptr(), ig.gamma.data_ptr()
            sj.h, sj.lat, sj.x_rounded, sj.bits = (o[k].data_ptr() for k in ("h", "lat", "x0", "lbits"))
            sj.a0, sj.h0, sj.y1 = (o[k].data_ptr() for k in ("a0", "h0", "y1"))
            sj.lat_row, sj.up0_row, sj.conv0_row = self._rows["latent"], self._rows["up0"], self._rows["conv0"]
            sj.mode, sj.ch, sj.c0, sj.c1 = (0 if stem_mode == "train" else 1), ch, c0, c1
            check(lib().nvf_step_head_stem(*args, ctypes.byref(sj), torch.cuda.current_stream().cuda_stream),
                  "nvf_step_head_stem")
        else:
            check(lib().nvf_step_head(*args, torch.cuda.current_stream().cuda_stream), "nvf_step_head")
        self._rate_ready = bool(with_rate)
        return dsts if stem_mode is None else dsts + [o]

    def prepare_weights(self, q):
        step, sd = self._noise()
        check(lib().nvf_prepare_weights(self.table.data_ptr(), self.nlayers, int(q), self.seed, step,
                                        None if sd is None else sd.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "nvf_prepare_weights")
        if self._mfma_jobs:
            ops.pack_mfma_all(self._mfma_jobs)      # conv1, conv2, up1, up2: every MFMA weight layout, one launch

    # ------------------------------------------------------------------ forward
    def _convT(self, L, x, act, train=False):
        r = routes.convT_fwd(self.decoder_class, self.winograd, L.name, L.cin, train)
        if r.form == "convT16":
            return ops.convT3d_k5s2_mfma16(x, L.wp[r.pack], L.b_eff, act, cout=L.cout, pad=L.pad)
        if r.form == "convT_mfma":
            return ops.convT3d_k5s2_mfma(x, L.wp[r.pack], L.b_eff, act, variant=r.variant)
        return ops.convT3d_k5s2_fwd(x, L.w_fwd, L.b_eff, L.cout, L.pad, act)

    def _conv(self, L, x, act, train=False):
        r = routes.conv_fwd(self.decoder_class, self.winograd, L.name, x.shape[0], train, act == R)
        if r.form == "wino16_fwd":
            return ops.conv3d_k4_wino16_fwd(x, L.wp[r.pack], L.b_eff)
        if r.form == "wino_fwd":
            return ops.conv3d_k4_wino_fwd(x, L.wp[r.pack], L.b_eff, ppc=r.ppc)
        if r.form == "g16":
            osz = tuple(s - 3 for s in x.shape[2:])
            return ops.conv3d_g16_mfma(x, L.wp[r.pack], L.b_eff, L.cout, 4, 1, 0, osz, act)
        if r.form == "k4_mfma":
            return ops.conv3d_k4_mfma(x, L.wp[r.pack], L.b_eff, 0, routes.PAIR_AXIS[r.pack], act, variant=r.variant)
        osz = tuple(s + 2 * L.pad - L.k + 1 for s in x.shape[2:])
        return ops.conv3d_gather(x, L.w_fwd, L.b_eff, L.cout, L.k, 1, L.pad, osz, act)

    def forward(self, e, mode, block_ids, defer_heads=False, stem=None, main_only=False):
        """e [B,ch,2,2,2] latents-before-latent_gen.  Returns the dict of saved activations.  ``defer_heads``: the caller
        runs backward() with weight gradients next -- at mini-batch sizes the heads' forward then rides in the launch of
        their loss and backward-data (a["p0"..] stay None until then).  ``stem``: the stem activations of this
        mini-batch that batch_and_prepare(..., stem_mode=mode) returned (None: forward() runs the stem itself).
        ``main_only``: conv2_cls alone of the three heads (a["p0"] = a["p1"] = None); backward(main_only=True) follows."""
        net, Ls = self.net, self.layers
        a = {"e": e}
        # (defer_heads is the caller's promise of a weight-gradient backward pass; backward() holds it to that)
        plan = self._plan(e.shape[0], want_w=defer_heads, step_head=stem is not None, defer_heads=defer_heads,
                          main_only=main_only)
        g2 = net.latent_gen.gdn_2
        ig = net.reconstructor.activation
        step, sd = self._noise()
        noise = dict(block_ids=block_ids, seed=self.seed, step=step, step_dev=sd)
        if plan.stem_fwd == "head":
            a.update(stem)                    # the step head's launch ran the latent generator, quantiser and stem
        elif plan.stem_fwd == "latent":       # latent generator, quantiser and stem in one launch
            (a["h"], a["lat"], a["x0"], a["lbits"], a["a0"], a["h0"], a["y1"]) = ops.stem_latent_fwd(
                e, Ls["latent"].w_fwd, Ls["latent"].b_eff, g2.beta, g2.gamma, *self._ec(), mode, Ls["up0"].w_fwd,
                Ls["up0"].b_eff, ig.beta, ig.gamma, Ls["conv0"].w_fwd, Ls["conv0"].b_eff, **noise)
        elif plan.latent_fwd_fused:           # latent generator + quantiser in one launch
            a["h"], a["lat"], a["x0"], a["lbits"] = ops.latent_fwd(
                e, Ls["latent"].w_fwd, Ls["latent"].b_eff, g2.beta, g2.gamma, *self._ec(), mode, **noise)
        else:
            a["h"] = self._conv(Ls["latent"], e, NONE)
            a["lat"] = ops.gdn_fwd(a["h"], g2.beta, g2.gamma, False)
            a["x0"], a["lbits"], _, _, _ = ops.latent_rate(a["lat"], *self._ec(), mode, **noise)
        if plan.stem_fwd == "fused":
            a["a0"], a["h0"], a["y1"] = ops.stem_fwd(a["x0"], Ls["up0"].w_fwd, Ls["up0"].b_eff, ig.beta, ig.gamma,
                                                     Ls["conv0"].w_fwd, Ls["conv0"].b_eff)
        elif plan.stem_fwd == "layers":
            a["a0"] = self._convT(Ls["up0"], a["x0"], NONE)
            a["h0"] = ops.gdn_fwd(a["a0"], ig.beta, ig.gamma, True)
            a["y1"] = self._convT(Ls["conv0"], a["h0"], R)
        if plan.heads == "layers":
            a["p0"] = self._conv(Ls["conv0_cls"], a["y1"], S)
        a["y2"] = self._convT(Ls["up1"], a["y1"], R, train=(mode == "train"))
        a["y3"] = self._conv(Ls["conv1"], a["y2"], R, train=(mode == "train"))
        if plan.heads == "layers":
            a["p1"] = self._conv(Ls["conv1_cls"], a["y3"], S)
        a["y4"] = self._convT(Ls["up2"], a["y3"], R, train=(mode == "train"))
        a["y5"] = self._conv(Ls["conv2"], a["y4"], R, train=(mode == "train"))
        if plan.heads == "deferred":
            a["p0"] = a["p1"] = a["p2"] = None      # nvf_heads3_fwd_loss_bwd_data (backward)
        elif plan.heads == "main":
            a["p0"] = a["p1"] = None
            a["p2"] = self._conv(Ls["conv2_cls"], a["y5"], S)
        elif plan.heads != "layers":                # all three heads in one launch, after the trunk
            hl = [Ls["conv0_cls"], Ls["conv1_cls"], Ls["conv2_cls"]]
            a["p0"], a["p1"], a["p2"] = ops.heads3_fwd([a["y1"], a["y3"], a["y5"]], [L.w_fwd for L in hl],
                                                       [L.b_eff for L in hl])
        else:
            a["p2"] = self._conv(Ls["conv2_cls"], a["y5"], S)
        return a

    # ------------------------------------------------------------------ backward
    def _wgrad_conv(self, L, g_out, x_in, sums):
        r = routes.conv_wgrad(self.decoder_class, self.winograd, L.name)
        if r.form == "wino16_partial":
            base = self._wg.reserve(256 * 16384 * 4)
            n = ops.wgrad16_k4_wino_partial(g_out, x_in, base, zsplit=r.zsplit)
            self._wg.add_job(base, L.gk, n, 16384)
        else:
            self._wg.add(g_out, x_in, L.k, 1, L.pad, 0, L.gk)
        sums.append((g_out, L.gb))

    def _wgrad_convT(self, L, g_out, x_in, sums):
        self._wg.add(x_in, g_out, 5, 2, L.pad, 0, L.gk)
        sums.append((g_out, L.gb))

    def _dx_conv(self, L, g_out, x_in, mask=None, addend=None, bias_out=None, sums=None):
        """Backward-data of a 4^3 convolution.  ``bias_out``: the bias gradient of the layer BELOW (whose masked output
        gradient dx this pass writes).  Where the matrix-core kernel leaves dx's channel sums as slabs, they become a job of
        the reduction launch; everywhere else (dx, bias_out) joins ``sums``, the step's list for the channel-sum pass."""
        r = routes.conv_dx(self.decoder_class, self.winograd, L.name, g_out.shape[0], mask is not None, addend is not None,
                           bias_out is not None)
        wp = L.wp.get(r.pack)
        if r.form == "wino16_bwd":
            dx = ops.conv3d_k4_wino16_bwd(g_out, wp, mask)
        elif r.form == "g16":
            dx = ops.conv3d_g16_mfma(g_out, wp, None, L.cin, 4, 1, 3, tuple(x_in.shape[2:]), addend=addend, mask=mask)
        elif r.form == "wino_bwd" and r.bias_slabs:
            base = self._wg.reserve(16384 * 8 * 4)
            dx, nparts = ops.conv3d_k4_wino_bwd(g_out, wp, mask, bias_part=base)
            self._wg.add_job(base, bias_out, nparts, 8)
        elif r.form == "wino_bwd":
            dx = ops.conv3d_k4_wino_bwd(g_out, wp, mask, ppc=r.ppc)
        elif r.form == "k4_mfma" and r.bias_slabs:
            base = self._wg.reserve(4096 * 8 * 4)
            dx, nparts = ops.conv3d_k4_mfma(g_out, wp, None, 3, routes.PAIR_AXIS[r.pack], NONE, mask=mask, bias_part=base)
            self._wg.add_job(base, bias_out, nparts, 8)
        elif r.form == "k4_mfma":
            dx = ops.conv3d_k4_mfma(g_out, wp, None, 3, routes.PAIR_AXIS[r.pack], NONE, addend=addend, mask=mask)
        else:
            dx = ops.conv3d_gather(g_out, L.w_bwd, None, L.cin, L.k, 1, L.k - 1 - L.pad, tuple(x_in.shape[2:]),
                                   addend=addend, mask=mask)
        if bias_out is not None and not r.bias_slabs:
            sums.append((dx, bias_out))
        return dx

    def _dx_convT(self, L, g_out, x_in, mask=None, addend=None):
        r = routes.convT_dx(self.decoder_class, self.winograd, L.name, L.cin, g_out.shape[0])
        if r.form == "g16":
            return ops.conv3d_g16_mfma(g_out, L.wp[r.pack], None, L.cin, 5, 2, L.pad, tuple(x_in.shape[2:]), addend=addend,
                                       mask=mask)
        if r.form == "s2k5_mfma":
            return ops.conv3d_s2k5_mfma(g_out, L.wp[r.pack], L.cin, addend=addend, mask=mask, variant=r.variant)
        return ops.conv3d_gather(g_out, L.w_bwd, None, L.cin, 5, 2, L.pad, tuple(x_in.shape[2:]), addend=addend,
                                 mask=mask)

    def _abandon_step(self):
        """The step in flight will not finish: forget everything it left for its later launches.  After any exception
        out of train_step, latent_step, eval_forward or backward the engine is in the state "no step in flight", and its
        next step is the bits of an engine that never failed.  Nothing queued in the context (final passes, stem
        backward, latent tail), no reduction job and no slab of the WgradBatch (a next step would append its jobs behind
        them, leave the one-launch reduction at more than 16 jobs and add stale slabs into its gradients), none of the
        flags one phase of a step leaves for a later one.  noise_step stays as bumped: the draw is spent.  What a
        launch already did on the device needs no repair: every cooperative launch returns its arrival counters to
        zero itself, and every buffer is written before it is read in the next step."""
        self.ctx.cancel()
        if self._wg is not None:
            self._wg.abandon()
        self._rate_ready = self.tail_done = False

    @_abandons_step
    def backward(self, a, gt, dist, gt16, gt8, n_pts, mode, block_ids, want_w, want_emb, fuse=None, main_only=False):
        """Loss (NVFPCC.py:161-196) and its gradients.  Weight grads land in self.flat_g.  The phases run in launch order;
        what they return stays referenced here until the last launch has been enqueued (queued stages write it late)."""
        deferred = a.get("p2") is None
        plan = self._plan(a["e"].shape[0], want_w, want_emb, fuse is not None, defer_heads=deferred, main_only=main_only)
        if deferred and plan.heads != "deferred":
            raise ValueError("forward(defer_heads=True) must be followed by a backward pass with weight gradients "
                             "(want_w=True): the heads' forward runs in that pass's loss launch")
        if self._wg is None:
            # (wide decoder: 125 MiB of slabs at batch 16 -- a workspace that had to grow mid-step would be reallocated)
            self._wg = ops.WgradBatch(self.dev, nbytes=(256 if self.wide else 128) << 20, ctx=self.ctx)    # partial sums now, ONE reduction launch for all ten
        # [main, head0, head1, unused]; main-head-only: the coarse terms are not part of the objective and read 0
        loss = torch.zeros(4, device=self.dev) if plan.heads == "main" else torch.empty(4, device=self.dev)
        nbits = torch.empty(7, device=self.dev)
        # the one-block final passes of the focal terms, the bias sums and the weight rate feed nothing inside the
        # step: queue them and run all three in one launch at the end
        if want_w:
            self.ctx.begin()
        sums = []       # (tensor, bias gradient): the channel sums still to take, in the order the reduction gets them
        t0, t1, g5, heads_job = self._bwd_loss_heads(plan, a, gt, dist, gt16, gt8, loss, sums)
        g4, g3, g2, g1 = self._bwd_trunk(plan, a, t0, t1, g5, sums)
        da0, dx0, stem_jobs = self._bwd_stem(plan, a, g1, sums)
        de, tail = self._bwd_latent(plan, a, dx0, n_pts, mode, block_ids, sums)
        sums_done = False
        if plan.trunk5:
            # conv2 / up2 / conv1 weight gradients, the longest launch of the step, go last of the big kernels: the
            # queued latent tail (a 30 us chain of three dependent stages in ONE workgroup) runs as its first workgroup
            # and is hidden behind them instead of being the critical path of the slab reduction; up1's and conv0's
            # gradients (small VALU kernels) fill the slots that the short matrix-core workgroups leave
            Ls = self.layers
            sums_done = plan.sums_in_trunk5 and self._rate_ready
            self._wg.add_trunk5([g5, a["y3"], g3, a["y1"], a["h0"]], [a["y4"], g4, a["y2"], g2, g1],
                                [Ls["conv2"].gk, Ls["up2"].gk, Ls["conv1"].gk, Ls["up1"].gk, Ls["conv0"].gk],
                                bias_outs=(Ls["conv2"].gb, Ls["conv1"].gb), heads=heads_job,
                                sums=([t for t, _ in sums], [o for _, o in sums]) if sums_done else None,
                                coef=((fuse["coef_dev"], self._coef_live)
                                      if (fuse is not None and fuse.get("coef_dev") is not None) else None),
                                stem_jobs=stem_jobs)
        last = {"loss_terms": loss, "latent_bits": a["lbits"], "net_bits": nbits, "n_pts": n_pts}
        self._bwd_finish(plan, sums, sums_done, last, fuse)
        self.last = last
        return de

    def _bwd_loss_heads(self, plan, a, gt, dist, gt16, gt8, loss, sums):
        """The three focal terms, their logit gradients and the heads' backward-data.  Returns (t0, t1, g5, heads_job): the
        heads' share of dy1 / dy3, dy5, and the heads' weight-gradient job where add_trunk5 takes it (None: launched here)."""
        Ls = self.layers
        want_w = plan.want_w
        ctx = self.ctx if want_w else None
        hl = [Ls["conv0_cls"], Ls["conv1_cls"], Ls["conv2_cls"]]

        def step_metrics():
            # logging counts of NVFPCC.py:174-179, 190-221 (tp / ap / tn / an of the main output and of both heads at 0.5,
            # sse / denom at 0.6): one partial-sum launch, the final pass rides in the finals launch; nvf_step_tail turns
            # them into the per-step ratios behind the all-reduce
            if self.epoch_acc is not None and want_w:
                ops.metrics3([a["p2"], a["p0"], a["p1"]], [gt, gt8, gt16], [dist, None, None], 0.5, 0.6,
                             out=self.step_counts, ctx=ctx)
        bias_outs = [L.gb for L in hl] if plan.head_bias_in_loss else None
        terms = ([gt8, gt16, gt], [None, None, dist], [0.85, 0.85, 0.9], [0.0, 0.0, 1.0], [1, 2, 0], loss, [L.w_bwd for L in hl])
        if plan.heads == "main":
            # the one focal term of p2 and conv2_cls's backward-data; nothing reaches y1 / y3 from a head (t0 = t1 = None)
            dl2, = ops.focal_loss_multi([(a["p2"], gt, dist, 0.9, 1.0)], loss)
            return None, None, self._dx_conv(Ls["conv2_cls"], dl2, a["y5"], mask=a["y5"]), None
        if plan.heads == "deferred":
            # the heads' forward, the three focal terms, their logit gradients and the heads' backward-data: ONE launch
            # (forward() left p0 / p1 / p2 to this call)
            (a["p0"], a["p1"], a["p2"]), (dl0, dl1, dl2), (t0, t1, g5) = ops.heads3_fwd_loss_bwd_data(
                [a["y1"], a["y3"], a["y5"]], [L.w_fwd for L in hl], [L.b_eff for L in hl], *terms, [None, None, a["y5"]],
                self.ctx, bias_outs=bias_outs)
            step_metrics()
        elif plan.heads == "fused_loss":    # the three focal terms, their logit gradients and the heads' backward-data: one launch
            step_metrics()
            (dl0, dl1, dl2), (t0, t1, g5) = ops.heads3_loss_bwd_data(
                [a["p0"], a["p1"], a["p2"]], *terms, [L.cin for L in hl], [None, None, a["y5"]], ctx=ctx, bias_outs=bias_outs)
        else:
            dl2, dl0, dl1 = ops.focal_loss_multi([(a["p2"], gt, dist, 0.9, 1.0), (a["p0"], gt8, None, 0.85, 0.0),
                                                  (a["p1"], gt16, None, 0.85, 0.0)], loss, ctx=ctx)
            step_metrics()
        if plan.heads == "layers":
            t1 = self._dx_conv(Ls["conv1_cls"], dl1, a["y3"])
            t0 = self._dx_conv(Ls["conv0_cls"], dl0, a["y1"])
            if want_w:
                self._wgrad_conv(Ls["conv2_cls"], dl2, a["y5"], sums)
                self._wgrad_conv(Ls["conv1_cls"], dl1, a["y3"], sums)
                self._wgrad_conv(Ls["conv0_cls"], dl0, a["y1"], sums)
            g5 = self._dx_conv(Ls["conv2_cls"], dl2, a["y5"], mask=a["y5"])
            return t0, t1, g5, None
        if plan.heads == "heads3":
            t0, t1, g5 = ops.heads3_bwd_data([dl0, dl1, dl2], [L.w_bwd for L in hl], [L.cin for L in hl],
                                             [None, None, a["y5"]])
        heads_job = None
        if want_w:
            heads_job = ([dl0, dl1, dl2], [a["y1"], a["y3"], a["y5"]], [L.gk for L in hl])
            if not plan.heads_in_trunk5:
                self._wg.add_heads3(*heads_job)
                heads_job = None
            if not plan.head_bias_in_loss:
                sums += [(dl2, hl[2].gb), (dl1, hl[1].gb), (dl0, hl[0].gb)]
        return t0, t1, g5, heads_job

    def _bwd_trunk(self, plan, a, t0, t1, g5, sums):
        """The backward-data chain g4 .. g1; each layer's weight gradient is issued as soon as its output gradient exists,
        except with plan.trunk5 (one launch, add_trunk5): up2's / up1's bias gradients = the channel sums of g4 / g2 then."""
        Ls = self.layers
        each = plan.want_w and not plan.trunk5
        if each:
            self._wgrad_conv(Ls["conv2"], g5, a["y4"], sums)
        g4 = self._dx_conv(Ls["conv2"], g5, a["y4"], mask=a["y4"], bias_out=Ls["up2"].gb if plan.trunk5 else None, sums=sums)
        if each:
            self._wgrad_convT(Ls["up2"], g4, a["y3"], sums)
        g3 = self._dx_convT(Ls["up2"], g4, a["y3"], mask=a["y3"], addend=t1)
        if each:
            self._wgrad_conv(Ls["conv1"], g3, a["y2"], sums)
        g2 = self._dx_conv(Ls["conv1"], g3, a["y2"], mask=a["y2"], bias_out=Ls["up1"].gb if plan.trunk5 else None, sums=sums)
        if each:
            self._wgrad_convT(Ls["up1"], g2, a["y1"], sums)
        g1 = self._dx_convT(Ls["up1"], g2, a["y1"], mask=a["y1"], addend=t0)
        if plan.trunk5 or plan.conv0_wgrad_in_stem:      # conv0's weight gradient: in add_trunk5 / in the stem's backward
            sums.append((g1, Ls["conv0"].gb))
        elif plan.want_w:
            self._wgrad_convT(Ls["conv0"], g1, a["h0"], sums)
        return g4, g3, g2, g1

    def _gdn_grads(self, prefix, mod, want_w):
        """(d beta, d gamma) views of a GDN's parameter gradients in flat_g, or (None, None) without weight gradients."""
        if not want_w:
            return None, None
        return self._g(prefix + ".beta"), self._g(prefix + ".gamma").view(mod.gamma.shape)

    def _bwd_stem(self, plan, a, g1, sums):
        """conv0^T -> IGDN' -> up0^T with up0's (and, plan.conv0_wgrad_in_stem, conv0's) gradients.  Returns (da0, dx0,
        stem_jobs): the reduction jobs of a queued stem for add_trunk5, else None."""
        Ls = self.layers
        ig = self.net.reconstructor.activation
        dbeta, dgamma = self._gdn_grads("reconstructor.activation", ig, plan.want_w)
        if plan.stem_bwd == "queued":
            # no launch here: queued in the context, it runs inside add_trunk5's launch (with the latent tail that
            # consumes dx0), which also takes its reduction jobs; up0's bias gradient comes from per-block channel sums
            # the stage leaves, not from da0
            return ops.stem_bwd_queue(g1, a["x0"], a["a0"], Ls["conv0"].w_bwd, Ls["up0"].w_bwd, ig.beta, ig.gamma, dbeta,
                                      dgamma, Ls["up0"].gk, Ls["up0"].gb, self.ctx)
        if plan.stem_bwd == "partial":          # its final launch is shared with the slab reduction / the final passes
            wg0 = plan.conv0_wgrad_in_stem
            da0, dx0 = ops.stem_bwd_partial(g1, a["x0"], a["a0"], Ls["conv0"].w_bwd, Ls["up0"].w_bwd, ig.beta,
                                            ig.gamma, dbeta, dgamma, Ls["up0"].gk, self._wg, ctx=self.ctx,
                                            h0=a["h0"] if wg0 else None, dw_conv0=Ls["conv0"].gk if wg0 else None)
            sums.append((da0, Ls["up0"].gb))
        elif plan.stem_bwd == "plain":
            da0, dx0 = ops.stem_bwd(g1, a["x0"], a["a0"], Ls["conv0"].w_bwd, Ls["up0"].w_bwd, ig.beta, ig.gamma)
        else:
            dh0 = self._dx_convT(Ls["conv0"], g1, a["h0"])
            da0, _, _ = ops.gdn_bwd(a["a0"], ig.beta, ig.gamma, dh0, True, dbeta, dgamma)
            if plan.want_w:
                self._wgrad_convT(Ls["up0"], da0, a["x0"], sums)
            dx0 = self._dx_convT(Ls["up0"], da0, a["x0"])
        return da0, dx0, None

    def _bwd_latent(self, plan, a, dx0, n_pts, mode, block_ids, sums):
        """Latent rate (+ the decoder's gradient through the straight-through round), the latent GDN and the 1x1x1 layer.
        Returns (de, tail): the latent gradient (plan.want_emb), and the tensors of a queued tail."""
        Ls = self.layers
        want_w = plan.want_w
        step, sd = self._noise()
        g_lat = self.lmbda * self.w1 / n_pts if self._g_lat_dev is None else 1.0
        g2m = self.net.latent_gen.gdn_2
        dsigma, dmu = (self._g("entropy_coder.sigma"), self._g("entropy_coder.mu")) if want_w else (None, None)
        dbeta, dgamma = self._gdn_grads("latent_gen.gdn_2", g2m, want_w)
        if plan.tail_queued:
            # three dependent launches on [B, ch, 2^3] tensors -> one workgroup of the next weight-gradient launch
            # (or of the slab reduction); dlat / dh / dx0 stay referenced until that launch has been enqueued
            dlat, dh = torch.empty_like(a["lat"]), torch.empty_like(a["h"])
            ops.latent_tail_queue(self.ctx, a["lat"], *self._ec(), mode, block_ids, dx0, dlat, dsigma, dmu,
                                  self._g_lat_dev, g_lat, self.seed, step, sd, a["h"], g2m.beta, g2m.gamma, dh, dbeta,
                                  dgamma, a["e"], Ls["latent"].gk, Ls["latent"].gb)
            return None, (dlat, dh)
        _, _, dlat, _, _ = ops.latent_rate(a["lat"], *self._ec(), mode, block_ids=block_ids, want_grad=True, g_host=g_lat,
                                           g_dev=self._g_lat_dev, seed=self.seed, step=step, step_dev=sd,
                                           dx_addend=dx0, dsigma_out=dsigma, dmu_out=dmu)
        dh, _, _ = ops.gdn_bwd(a["h"], g2m.beta, g2m.gamma, dlat, False, dbeta, dgamma)
        if want_w:
            self._wgrad_conv(Ls["latent"], dh, a["e"], sums)
        return (self._dx_conv(Ls["latent"], dh, a["e"]) if plan.want_emb else None), None

    def _bwd_finish(self, plan, sums, sums_done, last, fuse):
        """Weight rate (bits of the 7 quantised kernels and, for the decoder update, their gradients, added to the weight
        gradients), slab reduction, bias sums, final passes and -- single GPU -- the optimiser.  ``sums_done``: the partial
        bias sums rode in add_trunk5."""
        Ls, nbits = self.layers, last["net_bits"]
        lm = self.net.reconstructor.likelihood_model
        kernels = [Ls[n].mod.kernel for n in TRUNK]
        rate_head, self._rate_ready = self._rate_ready and plan.want_w, False
        self.tail_done = False
        if not plan.want_w:
            ops.weight_rate_batch(kernels, None, lm.sigma, lm.mu, nbits)
            return
        gs, gm = self._g("reconstructor.likelihood_model.sigma"), self._g("reconstructor.likelihood_model.mu")
        addends = fused = None
        if rate_head:
            # the weight-rate gradient was computed by the step head: the reduction adds it while it writes the
            # gradients (every trunk kernel must come out of that launch; otherwise the stand-alone pass)
            job, addends = self._rate_job()[:2]
            live = {out for out, _ in self._wg.live_outputs()}
            if not all(Ls[n].gk.data_ptr() in live for n in TRUNK) or len(self._wg.jobs) > 16:
                rate_head, addends = False, None
        if plan.fused_optimiser and rate_head:
            fused = tail, adam, ranges = self._fused_tail(plan, fuse, sums, last, gs, gm)
            self.tail_done = True
        # nothing the final passes read is written by the slab reduction: ONE launch for both where the bias partials exist
        one_launch = sums_done and rate_head
        todo = [] if sums_done else sums
        if not one_launch and not fused:
            self._wg.finish_with_sums([t for t, _ in todo], [o for _, o in todo], addends=addends)
        if rate_head:
            ops.weight_rate_final(job, nbits, gs, gm, ctx=self.ctx)
        else:
            g_net = self.lmbda * self.w2 / self.n_points_total
            ops.weight_rate_batch(kernels, [Ls[n].gk for n in TRUNK], lm.sigma, lm.mu, nbits, gs, gm,
                                  g_host=g_net * self.rate_grad_scale, ctx=self.ctx)
        if one_launch and fused:
            if fuse.get("coef_dev") is not None:     # the copy add_trunk5 staged: not the step buffer's words
                adam.coef_dev = self._coef_live.data_ptr()
            self._wg.finish_and_flush_tail(addends, adam, tail, ranges)
        elif one_launch:    # data parallelism (the all-reduce and the step tail follow): the same pairing without the optimiser
            self._wg.finish_and_flush(addends)
        elif fused:
            # the optimiser is split over the slab reduction (weight gradients) and the finals launch (the rest): both
            # launches in ONE library call, so that no exception between them leaves the parameters half updated
            self._wg.finish_with_sums([t for t, _ in todo], [o for _, o in todo], addends=addends, adam=adam, tail=tail,
                                      ranges=ranges)
        else:
            self.ctx.flush()

    def _tail_kw(self, last):
        """The step_tail arguments every form of the optimiser tail shares: the optimiser state, the statistics inputs of
        the step ``last`` (only while epoch statistics are on), the accumulators and the arrival counter."""
        stats = self.epoch_acc is not None
        return dict(p=self.flat_p, g=self.flat_g, m=self.flat_m, v=self.flat_v,
                    loss_terms=last["loss_terms"] if stats else None, lbits=last["latent_bits"] if stats else None,
                    nbits=last["net_bits"] if stats else None, nbits_scale=1.0 / self.n_points_total,
                    counts=self.step_counts if stats else None, acc=self.epoch_acc, done=self._tail_done)

    def _fused_tail(self, plan, tail, sums, last, gs, gm):
        """(NvfStepTail, NvfAdamFuse, uncovered ranges) for a step whose optimiser rides in the slab reduction (weight
        gradients) and in the finals launch (everything those final passes write + the ranges): single-GPU steps only.
        ``tail``: dict(coef_dev= / coef_host=, inv_npts_dev= / inv_npts_host=, sched=)."""
        t = ops.step_tail_args(**tail, **self._tail_kw(last))
        outs = [o for _, o in sums] + [gs, gm]
        if plan.head_bias_in_loss:      # written by the loss launch's own final pass (no channel-sum job)
            outs += [self.layers[n].gb for n in ("conv0_cls", "conv1_cls", "conv2_cls")]
        if plan.stem_bwd in ("queued", "partial"):      # the stem's IGDN gradients: a deferred final pass
            outs += [self._g("reconstructor.activation.beta"), self._g("reconstructor.activation.gamma")]
        base = self.flat_g.data_ptr()
        cover = [((ptr - base) // 4, (ptr - base) // 4 + cnt)
                 for ptr, cnt in self._wg.live_outputs() + [(o.data_ptr(), o.numel()) for o in outs]]
        n = self.flat_g.numel()
        key = tuple(sorted(c for c in cover if 0 <= c[0] < n))
        ranges = self._tail_ranges.get(key)
        if ranges is None:
            ranges, pos = [], 0
            for lo, hi in key:
                if lo < pos:
                    raise RuntimeError("fused tail: two launches write the same gradient elements")
                if lo > pos:
                    ranges.append((pos, lo))
                pos = hi
            if pos < n:
                ranges.append((pos, n))
            if len(ranges) > 16:
                raise RuntimeError("fused tail: more than 16 uncovered gradient ranges")
            self._tail_ranges[key] = ranges
        return t, ops.adam_fuse_args(t), ranges

    # ------------------------------------------------------------------ steps
    def _batch(self, idx_dev):
        """(gt, dist, gt16, gt8, emb) rows of the mini-batch: one fused gather."""
        return ops.gather_rows_multi([self.gt, self.dist, self.gt16, self.gt8, self.emb], idx_dev)

    def enable_epoch_stats(self):
        """Device accumulators behind NVFPCC.py train's per-epoch log line (the reference syncs ~14 .item()s per step,
        NVFPCC.py:190-221): epoch_acc[16] = the three focal terms, b_latent, b_net, non-finite objective terms,
        non-finite gradient entries, steps, then the per-step ratios Pacc, Nacc, S1Pacc, S1Nacc, S2Pacc, S2Nacc summed
        over the steps, sse, denom (nvf_step_tail)."""
        if self.epoch_acc is None:
            self.epoch_acc = torch.zeros(16, device=self.dev)

    def read_epoch_stats(self, reset=True, reduce=None, world=1):
        """epoch_acc as a float64 numpy array [16]: ONE host sync per epoch.  ``reduce``: the data-parallel SUM
        all-reduce, applied to the 16 floats first; entries that every rank holds identically (b_net, the step count and
        the ratios / sse / denom, which nvf_step_tail derives from all-reduced counts) are divided by ``world`` after it.
        Raises on the reference's NaN checks (NVFPCC.py:199-212: 'Problem in loss' / 'Problem with grad') instead of
        opening an IPython shell; a non-finite gradient entry never reaches its parameter (nvf_step_tail skips it)."""
        acc = self.epoch_acc.clone()
        if reduce is not None:
            reduce(acc)
        acc = acc.double().cpu().numpy()
        if reduce is not None and world > 1:
            acc[4] /= world
            acc[7:16] /= world
        if reset:
            self.epoch_acc.zero_()
        if acc[5] > 0:
            raise ValueError("Problem in loss: %d non-finite objective terms this epoch" % int(acc[5]))
        if acc[6] > 0:
            raise ValueError("Problem with grad: %d non-finite gradient entries this epoch" % int(acc[6]))
        return acc

    def train_log_fields(self, acc, nsteps, peak=1023):
        """The 16 numbers of the reference's TRAIN line after 'seconds]' (NVFPCC.py:261-281), from read_epoch_stats:
        Loss, PosiPenal, PosiGain, Pacc, Nacc, S1 Loss, S2 Loss, S1Pacc, S1Nacc, S2Pacc, S2Nacc, bpp, b_latent, b_net,
        MSE1, PSNR1 -- means over the epoch's mini-batches, MSE1 = sum sse / sum denom (0 / 0 = nan, as there).  peak:
        2^bits - 1 of the cloud, the peak of PSNR1."""
        cnt = float(nsteps)
        ls, bl, bn = acc[0:3] / cnt, acc[3] / cnt, acc[4] / cnt
        with np.errstate(divide="ignore", invalid="ignore"):
            mse1 = np.float64(acc[14]) / np.float64(acc[15])
            psnr1 = 20 * np.log10(peak / np.sqrt(mse1 / 3))
        loss = ls.sum() + self.lmbda * (bl * self.w1 + bn * self.w2)
        return [loss, 0.0, 0.0, acc[8] / cnt, acc[9] / cnt, ls[1], ls[2], acc[10] / cnt, acc[11] / cnt,
                acc[12] / cnt, acc[13] / cnt, bl + bn, bl, bn, mse1, psnr1]

    def _tail(self, n_pts):
        """All-reduce hook (data parallelism), then Adam (+ the epoch sums): nvf_step_tail with host coefficients."""
        if self.grad_hook is not None:
            self.grad_hook(self.flat_gx)
        ops.step_tail(coef_host=ops.adam_coefficients(self.lr, self.opt_step + 1), inv_npts_host=1.0 / n_pts,
                      **self._tail_kw(self.last))
        self.opt_step += 1         # (behind the launch: a step whose optimiser did not run has not happened)

    def _idle_backward(self):
        """A rank whose share of a short last mini-batch is empty (NVFPCC.py:149 with 917 mod 16 = 5 blocks on 8
        GPUs): no block terms, but its 1/W share of the replicated weight-rate gradient (and of d/d sigma, d/d mu of
        the likelihood model) still goes into the all-reduce, so the summed gradient is the single-GPU one."""
        net, Ls = self.net, self.layers
        self.flat_gx.zero_()
        lm = net.reconstructor.likelihood_model
        nbits = torch.empty(7, device=self.dev)
        g_net = self.lmbda * self.w2 / self.n_points_total
        ops.weight_rate_batch([Ls[n].mod.kernel for n in TRUNK], [Ls[n].gk for n in TRUNK], lm.sigma, lm.mu, nbits,
                              self._g("reconstructor.likelihood_model.sigma"),
                              self._g("reconstructor.likelihood_model.mu"), g_host=g_net * self.rate_grad_scale)
        self.last = {"loss_terms": torch.zeros(4, device=self.dev), "latent_bits": torch.zeros(1, device=self.dev),
                     "net_bits": nbits, "n_pts": 1.0}

    @_abandons_step
    def train_step(self, idx_host, q, idx_dev=None, update=True, n_pts=None):
        """One mini-batch decoder update (NVFPCC.py:149-223, minus logging).  Under data parallelism
        ``idx_host`` is this rank's share of the global mini-batch (possibly empty) and ``n_pts`` the occupied-voxel
        count of the WHOLE mini-batch (host-known: every rank derives the same epoch order)."""
        idx_host = np.asarray(idx_host, np.int64)
        self.noise_step += 1       # a fresh draw per train-mode forward whatever q is (latent noise, network.py:4516)
        a = None
        if idx_host.shape[0] == 0:
            self._idle_backward()
            n_pts = 1.0
        else:
            if idx_dev is None:
                idx_dev = torch.from_numpy(idx_host).to(self.dev)
            if n_pts is None:
                n_pts = float(self.counts[idx_host].sum())
            gt, dist, gt16, gt8, e, stem = self.batch_and_prepare(idx_dev, q, with_rate=True, stem_mode="train")
            a = self.forward(e, "train", idx_dev, defer_heads=True, stem=stem)
            tail = None
            if update and self.grad_hook is None:
                # single GPU: the optimiser rides in the slab reduction and the finals launch (no all-reduce in between)
                tail = dict(coef_host=ops.adam_coefficients(self.lr, self.opt_step + 1), inv_npts_host=1.0 / n_pts)
            self.backward(a, gt, dist, gt16, gt8, n_pts, "train", idx_dev, want_w=True, want_emb=False, fuse=tail)
            if tail is not None and self.tail_done:
                self.opt_step += 1
                update = False
        if update:
            self._tail(n_pts)
        elif self.grad_hook is not None:
            self.grad_hook(self.flat_gx)
        return a

    @_abandons_step
    def latent_step(self, q, lo=0, hi=None, update=True):
        """Full-batch latent update over blocks [lo, hi) (NVFPCC.py:225-251); no weight gradients."""
        hi = self.N_leaf if hi is None else hi
        self.noise_step += 1
        self.prepare_weights(q)
        a, de = self._latent_grad(lo, hi)
        if update:
            self._latent_update(lo, hi, de)
        return a, de

    def _latent_grad(self, lo, hi, main_only=False):
        """Forward and latent gradient of blocks [lo, hi) at the noise counter and the effective weights as they stand.
        The noise of a block is keyed by its absolute id (block_ids), not by its place in the batch, and every loss term
        is a sum over blocks: the rows of `de` do not depend on which other blocks share the pass.  ``main_only``: the
        objective is the main output's focal term plus the latent rate (plan_step)."""
        ids = torch.arange(lo, hi, device=self.dev)
        n_pts = float(self.counts.sum())          # the reference divides by the points of ALL blocks
        a = self.forward(self.emb[lo:hi], "train", ids, main_only=main_only)
        de = self.backward(a, self.gt[lo:hi], self.dist[lo:hi], self.gt16[lo:hi], self.gt8[lo:hi], n_pts, "train",
                           ids, want_w=False, want_emb=True, main_only=main_only)
        return a, de

    def _latent_update(self, lo, hi, de):
        ops.adam_step(self.emb[lo:hi].view(-1), de.view(-1), self.emb_m[lo:hi].view(-1),
                      self.emb_v[lo:hi].view(-1), self.lr_emb, self.emb_step + 1)
        self.emb_step += 1

    @_abandons_step
    def latent_step_chunked(self, q, lo=0, hi=None, chunk=LATENT_CHUNK, update=True):
        """latent_step(q, lo, hi) with at most `chunk` blocks resident at a time: ONE draw of the noise counter, ONE
        prepare_weights and ONE Adam step number for all of [lo, hi), n_pts the points of ALL blocks, the forward and
        backward chunk by chunk (a group of frames multiplies the block count; the activations of a pass grow with
        it).  hi - lo <= chunk: latent_step itself.  Returns the latent gradient of [lo, hi)."""
        hi = self.N_leaf if hi is None else hi
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"latent_step_chunked: chunk = {chunk}")
        if hi - lo <= chunk:
            return self.latent_step(q, lo, hi, update)[1]
        self.noise_step += 1
        self.prepare_weights(q)
        de = torch.cat([self._latent_grad(c, min(c + chunk, hi))[1] for c in range(lo, hi, chunk)], 0)
        if update:
            self._latent_update(lo, hi, de)     # after the last chunk: no chunk sees rows another one has moved
        return de

    @_abandons_step
    def eval_forward(self, lo=0, hi=None, q=2):
        hi = self.N_leaf if hi is None else hi
        ids = torch.arange(lo, hi, device=self.dev)
        self.prepare_weights(q)
        return self.forward(self.emb[lo:hi], "eval", ids)

    def eval_sums(self, lo=0, hi=None, q=2):
        """Additive sums behind the TEST line (NVFPCC.py:308-364) over blocks [lo, hi): [0:3] the three focal terms,
        [3:21] the 18 metric counts of ops.metrics3 (main output, head 0, head 1), [21] the latent bits.  Every entry is a
        SUM over blocks, so a rank evaluates its contiguous shard and ONE all-reduce of these 22 floats gives the
        full-batch numbers (eval shards contiguously; the reference evaluates on one device)."""
        hi = self.N_leaf if hi is None else hi
        if hi - lo > LATENT_CHUNK:          # a shard beyond one resident pass: the 22 sums chunk by chunk, added in float64
            tot = torch.zeros(22, device=self.dev, dtype=torch.float64)
            for c in range(lo, hi, LATENT_CHUNK):
                tot += self.eval_sums(c, min(c + LATENT_CHUNK, hi), q).double()
            return tot.float()
        out = torch.zeros(22, device=self.dev)
        if hi <= lo:
            return out
        a = self.eval_forward(lo, hi, q)
        loss = torch.empty(4, device=self.dev)
        gt, dist, gt16, gt8 = self.gt[lo:hi], self.dist[lo:hi], self.gt16[lo:hi], self.gt8[lo:hi]
        ops.focal_loss_multi([(a["p2"], gt, dist, 0.9, 1.0), (a["p0"], gt8, None, 0.85, 0.0),
                              (a["p1"], gt16, None, 0.85, 0.0)], loss)
        c = ops.metrics3([a["p2"], a["p0"], a["p1"]], [gt, gt8, gt16], [dist, None, None], 0.5, 0.6)
        out[0:3] = loss[0:3]
        out[3:21] = c[0:18]
        out[21] = a["lbits"].reshape(-1)[0]
        return out

    # ------------------------------------------------------------------ latents under a frozen decoder
    def _block_sums(self, lo, hi):
        """float64 [hi - lo, 2]: (main focal sum, eval-mode latent bits) of every block of [lo, hi), by the eval forward
        at the effective weights as they stand, at most LATENT_CHUNK blocks resident at a time."""
        outs = []
        for c in range(lo, hi, LATENT_CHUNK):
            e = min(c + LATENT_CHUNK, hi)
            a = self.forward(self.emb[c:e], "eval", torch.arange(c, e, device=self.dev))
            outs.append(ops.block_costs(a["p2"], self.gt[c:e], self.dist[c:e], 0.9, 1.0, a["x0"], *self._ec()))
        return torch.cat(outs, 0) if outs else torch.zeros(0, 2, dtype=torch.float64, device=self.dev)

    def _cost(self, sums):
        """J_b = c_f * focal_b + c_r * bits_b in float64, with the coefficients the main-head-only latent gradient
        differentiates: the focal term enters the objective as it is (_bwd_loss_heads: its gradient is unscaled) and the
        latent bits times lambda * w1 / n_pts, n_pts the occupied voxels of ALL the engine's blocks (_latent_grad,
        _bwd_latent).  The weight-rate term does not depend on the latents and is left out."""
        c_f, c_r = 1.0, self.lmbda * self.w1 / float(self.counts.sum())
        return c_f * sums[:, 0] + c_r * sums[:, 1]

    @_abandons_step
    def block_costs(self, lo=0, hi=None):
        """Per-block cost J_b (float64 [hi - lo]) of the rounded latents of blocks [lo, hi) under the decoder at q = 2 --
        the route eval_forward takes.  Under frozen weights the objective of the latent fit is the plain sum of these: a
        block's cost depends on its own `emb` row only, and not on which blocks share the pass (nvf_block_costs)."""
        hi = self.N_leaf if hi is None else hi
        self.prepare_weights(2)
        return self._cost(self._block_sums(lo, hi))

    @_abandons_step
    def fit_latents(self, steps, eval_every=10, lo=0, hi=None, report=None):
        """Fit the latents of blocks [lo, hi) under the decoder as it stands, frozen at q = 2: ``steps`` main-head-only
        latent steps in "train" mode (fresh latent noise per step), Adam on `emb` alone.  No net parameter, neither Adam
        moment of the net and not opt_step moves; the weights carry no noise at q = 2 and are prepared once.

        Before the first step, after every ``eval_every``-th and after the last one the per-block costs are evaluated
        and every block keeps the `emb` row with the lowest J_b so far (strict <: the earlier row wins a tie).  This is
        valid because the decoder is frozen -- the objective is a sum of per-block costs, each a function of its own row
        -- so no block ends worse than it started.  At the end emb[lo:hi] holds the kept rows.  Returns (J_start,
        J_final), float64 [hi - lo].  ``report(step, J_kept, improved, bits_kept)``: called after every evaluation with
        device tensors (the kept costs, which blocks improved on the start, the kept rows' latent bits)."""
        hi = self.N_leaf if hi is None else hi
        steps, eval_every = int(steps), int(eval_every)
        if steps < 0 or eval_every < 1 or not 0 <= lo < hi <= self.N_leaf:
            raise ValueError(f"fit_latents: steps = {steps}, eval_every = {eval_every}, blocks [{lo}, {hi})")
        self.prepare_weights(2)
        kept = self.emb[lo:hi].clone()
        sums = self._block_sums(lo, hi)
        J0 = self._cost(sums)
        J, bits = J0.clone(), sums[:, 1].clone()
        if report is not None:
            report(0, J, J < J0, bits)
        for s in range(1, steps + 1):
            self.noise_step += 1
            de = torch.cat([self._latent_grad(c, min(c + LATENT_CHUNK, hi), main_only=True)[1]
                            for c in range(lo, hi, LATENT_CHUNK)], 0)
            self._latent_update(lo, hi, de)     # after the last chunk, as latent_step_chunked
            if s % eval_every == 0 or s == steps:
                sums = self._block_sums(lo, hi)
                Js = self._cost(sums)
                better = Js < J
                kept = torch.where(better.view(-1, 1, 1, 1, 1), self.emb[lo:hi], kept)
                J, bits = torch.where(better, Js, J), torch.where(better, sums[:, 1], bits)
                if report is not None:
                    report(s, J, J < J0, bits)
        self.emb[lo:hi] = kept
        return J0, J

    def weight_bits(self):
        """Sum of the 7 quantised kernels' rate terms (identical on every rank): host float, one sync."""
        nbits = torch.empty(7, device=self.dev)
        lm = self.net.reconstructor.likelihood_model
        ops.weight_rate_batch([self.layers[n].mod.kernel for n in TRUNK], None, lm.sigma, lm.mu, nbits)
        return float(nbits.sum().item())

    def loss_value(self):
        """Host scalar of the last step's objective (one sync; logging only)."""
        t = self.last
        terms = t["loss_terms"].cpu().numpy()
        b_latent = t["latent_bits"].item() / t["n_pts"]
        b_net = t["net_bits"].sum().item() / self.n_points_total
        return float(terms[0] + terms[1] + terms[2] + self.lmbda * (b_latent * self.w1 + b_net * self.w2))


class GraphedTrainStep:
    """The whole mini-batch step -- step head, forward, losses, backward, [all-reduce], Adam + epoch sums -- captured
    once into a HIP graph and replayed: removes ~90 host-side launches per step (the reference pays ~1 500 aten
    dispatches).  Everything that changes from step to step comes from device memory: block ids, the noise-step
    counter, the rate coefficient lambda*w1/n_pts (and 1/n_pts for the log line) and Adam's two step-dependent
    coefficients (lr / (1 - b1^t), sqrt(1 - b2^t)) are one ROW of a schedule the host uploads once per epoch
    (``load_schedule``); the last kernel of step s (nvf_step_tail) copies row s + 1 over the buffer the kernels read, so
    a replay costs the host one graph launch and the GPU no host-to-device copy.

    Data parallelism: ``collective`` = "graph" captures the all-reduce of the gradient buffer as a node of the graph
    (the hand-over between the compute stream and RCCL's stream is then a graph edge instead of two event waits per
    step); "host" ends the graph after the backward pass and launches the all-reduce hook and the optimiser node from
    the host.  The default is "host" (dist.attach leaves it there; NVF_GRAPH_COLLECTIVE=graph or collective="graph" opts in,
    falling back to "host" in-process if the capture fails)."""

    CAP = 4096       # rows of the device-resident schedule (longer schedules are loaded in pieces)
    # steps per replay of the unrolled graphs, largest first (a run of n loaded steps is replayed greedily: 57 = 3 x 16 + 8
    # + 1 is five graph launches; 20 = 16 + 4 two)
    UNROLL = (16, 8, 4, 2)

    def __init__(self, eng, batch, q, ring=2, collective=None, unroll=None):
        self.eng, self.batch, self.q = eng, batch, q
        un = self.UNROLL if unroll is None else ((unroll,) if isinstance(unroll, int) else tuple(unroll))
        self.unrolls = tuple(u for u in sorted({max(int(v), 1) for v in un}, reverse=True) if u > 1)
        self.unroll = self.unrolls[0] if self.unrolls else 1
        dev = eng.dev
        if collective is None:
            collective = getattr(eng, "collective_mode", None) or os.environ.get("NVF_GRAPH_COLLECTIVE", "host")
        self.collective = collective if eng.grad_hook is not None else "none"
        # the buffer the step's kernels read: [idx (B x i64) | noise step (u64) | lambda*w1/n_pts, 1/n_pts (2 x f32) |
        # Adam coefficients (2 x f32)]; sched = [cursor | unused | CAP + 1 rows of the same layout]
        # -- one allocation [step buffer | cursor | unused | rows], so that loading a schedule is ONE host-to-device copy
        nw = self.nw = batch + 3
        self.sched = torch.zeros(nw + 2 + (self.CAP + 1) * nw, dtype=torch.int64, device=dev)
        self.buf = self.sched[:nw]
        self.cursor, self.rows = self.sched[nw:nw + 1], self.sched[nw + 2:]
        # staging ring: the host may load the next schedule while the copy of the previous one has not executed yet
        self.pins = [torch.zeros(self.sched.numel(), dtype=torch.int64).pin_memory() for _ in range(max(int(ring), 1))]
        self.pin_np = [p.numpy() for p in self.pins]                    # the same memory, for the NumPy row fill
        self.pin_events = [None] * len(self.pins)
        self.pin_gen = [0] * len(self.pins)          # generation of each slot's contents (stale handles are refused)
        self.loads = 0
        self.pending = []            # (n_pts) of the loaded steps not replayed yet
        self.idx = self.buf[:batch]
        self.step = self.buf[batch:batch + 1]
        rate = self.buf[batch + 1:batch + 2].view(torch.float32)
        self.g_lat, self.inv_npts = rate[0:1], rate[1:2]
        self.coef = self.buf[batch + 2:batch + 3].view(torch.float32)
        eng._step_dev, eng._g_lat_dev = self.step, self.g_lat
        first = torch.zeros(nw, dtype=torch.int64)
        first[:batch] = torch.arange(batch) % eng.N_leaf
        first[batch + 1:batch + 2].view(torch.float32)[:] = 1.0
        self.buf.copy_(first)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        acc = eng.epoch_acc
        try:
            with torch.cuda.stream(side):      # warm-up: allocates the grow-only workspaces outside the graph; the
                for _ in range(2):             # tail (no workspace) is left out, so no state is touched
                    self._body(tail=False)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            if self.collective == "graph":
                try:
                    self._capture(True)
                except Exception as e:       # noqa: BLE001 -- a failed capture of the collective: host launch instead
                    import warnings
                    warnings.warn(f"all-reduce could not be captured into the step graph ({e}); launching it from "
                                  f"the host behind the graph instead")
                    torch.cuda.synchronize()
                    self.collective = eng.collective_mode = "host"
                    self._capture(False)
            else:
                self._capture(self.collective != "host")
        finally:
            eng._step_dev, eng._g_lat_dev = None, None

    def _capture(self, tail):
        """graph: one step.  graphs_u[u]: u steps back to back -- every step's last kernel hands the step buffer
        over to the next schedule row, so the bodies are identical; a graph launch costs ~9 us of idle GPU between two
        replays (measured: 461 us period against 452 us of kernels), which an unrolled graph pays once per u steps.
        Only when the optimiser is inside the graph (not with a host-launched all-reduce)."""
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body(tail=tail)
        self.eng._graphs_captured += 1
        self.out1, self.last1 = self.out, self.last          # each graph writes tensors of its own
        self.graphs_u = {}
        for u in (self.unrolls if tail else ()):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(u):
                    self._body(tail=tail)
            self.graphs_u[u] = (g, self.out, self.last)       # ... an unrolled one: those of its last step
        self.graph_u = self.graphs_u[self.unroll][0] if self.graphs_u else None

    def _body(self, tail):
        eng = self.eng
        gt, dist, gt16, gt8, e, stem = eng.batch_and_prepare(self.idx, self.q, with_rate=True, stem_mode="train")
        a = eng.forward(e, "train", self.idx, defer_heads=True, stem=stem)
        spec = None
        if tail and eng.grad_hook is None:      # single GPU: no launch of its own for the tail
            spec = dict(coef_dev=self.coef, inv_npts_dev=self.inv_npts, sched=(self.buf, self.rows, self.cursor, self.nw))
        eng.backward(a, gt, dist, gt16, gt8, 1.0, "train", self.idx, want_w=True, want_emb=False, fuse=spec)
        self.out = a
        self.last = dict(eng.last)
        if tail and not (spec is not None and eng.tail_done):
            self._tail()

    def _tail(self):
        eng = self.eng
        if eng.grad_hook is not None:
            eng.grad_hook(eng.flat_gx)
        ops.step_tail(coef_dev=self.coef, inv_npts_dev=self.inv_npts, sched=(self.buf, self.rows, self.cursor, self.nw),
                      **eng._tail_kw(self.last))

    def stage_schedule(self, steps):
        """Host half of load_schedule: validates `steps` and fills the rows (block ids, noise steps, rate and Adam
        coefficients continuing from the engine's counters) into a pinned staging buffer; nothing reaches the device and no
        engine state changes.  Returns a handle for load_schedule -- valid while the engine's step counters and learning rate
        stay what they were (a training loop can prepare the next epoch's schedule while the GPU still runs this one)."""
        eng, B, nw = self.eng, self.batch, self.nw
        # the arrays form is recognised by its first member being a 2-D ndarray (a tuple of two (ids, n_pts) pairs is a
        # two-step list, not the arrays form)
        def is2d(x):          # ndarray / tensor [n, B], or a sequence of 1-D rows ((ids, n_pts) has a scalar / None second member)
            if isinstance(x, np.ndarray) or torch.is_tensor(x):
                return x.ndim == 2
            return (isinstance(x, (list, tuple)) and len(x) > 0 and
                    all(isinstance(r, (list, tuple, np.ndarray)) and np.ndim(r) == 1 for r in x))
        arrays = len(steps) == 2 and is2d(steps[0])
        if arrays and torch.is_tensor(steps[0]):
            steps = (steps[0].cpu().numpy(), steps[1].cpu().numpy() if torch.is_tensor(steps[1]) else steps[1])
        if arrays:
            ids_all, npts = np.asarray(steps[0], np.int64), np.asarray(steps[1], np.float64)
        else:
            ids_all = np.stack([np.asarray(ids, np.int64).reshape(-1) for ids, _ in steps]) if len(steps) else np.zeros((0, B), np.int64)
            npts = np.array([float(eng.counts[ids_all[k]].sum()) if p is None else float(p)
                             for k, (_, p) in enumerate(steps)], np.float64)
        n = ids_all.shape[0]
        if not (0 < n <= self.CAP):
            raise ValueError("load_schedule: 1..%d steps" % self.CAP)
        if ids_all.shape != (n, B) or npts.shape != (n,):
            raise ValueError("load_schedule: ids must be [n, %d] and n_pts [n]; got %s, %s" % (B, ids_all.shape, npts.shape))
        slot = self.loads % len(self.pins)
        self.loads += 1
        if self.pin_events[slot] is not None:
            self.pin_events[slot].synchronize()
        host = self.pin_np[slot]
        # the rows are filled as ONE NumPy array (per-element writes into a torch tensor cost ~10 us each: milliseconds per
        # epoch of host time that a short timed region would see)
        rows = host[nw + 2:nw + 2 + (n + 1) * nw].reshape(n + 1, nw)      # written in place (pinned memory)
        f32 = rows.view(np.float32)               # [n + 1, 2 nw]
        rows[:n, :B] = ids_all
        rows[:n, B] = eng.noise_step + 1 + np.arange(n)
        f32[:n, 2 * (B + 1)] = (eng.lmbda * eng.w1 / npts).astype(np.float32)
        f32[:n, 2 * (B + 1) + 1] = (1.0 / npts).astype(np.float32)
        f32[:n, 2 * (B + 2):2 * (B + 2) + 2] = ops.adam_coefficients_n(eng.lr, eng.opt_step + 1, n)
        rows[n] = rows[n - 1]                     # what the last step's tail copies (never used)
        host[:nw] = rows[0]                       # the step buffer starts as row 0 ...
        host[nw], host[nw + 1] = 1, 0             # ... and the cursor at 1: the tail of the first step fetches row 1
        self.pin_gen[slot] += 1                   # a handle owns its slot only until the slot is staged again
        m = nw + 2 + (n + 1) * nw
        return {"_staged": True, "slot": slot, "gen": self.pin_gen[slot], "n": n, "npts": npts.tolist(), "words": m,
                "src": self.pins[slot][:m], "dst": self.sched[:m],          # (sliced here, not inside a timed region)
                "state": (eng.noise_step, eng.opt_step, eng.lr, eng.lmbda, eng.w1)}

    def load_schedule(self, steps):
        """steps: [(block ids of this rank [batch], n_pts of the whole mini-batch or None)] in replay order (at most
        CAP) -- or the same as two arrays (ids [n, batch] int64 ndarray, n_pts [n] ndarray) -- or a handle from
        stage_schedule.  One host-to-device copy for all of them; Adam / noise counters continue from the engine's.
        Nothing is touched before the input has been validated."""
        eng = self.eng
        if self.pending:
            raise ValueError("load_schedule: only after every loaded step has been replayed")
        h = steps if (isinstance(steps, dict) and steps.get("_staged")) else self.stage_schedule(steps)
        if h["state"] != (eng.noise_step, eng.opt_step, eng.lr, eng.lmbda, eng.w1):
            raise ValueError("load_schedule: the staged schedule was made for other step counters / coefficients")
        slot, m = h["slot"], h["words"]
        if h.get("gen") != self.pin_gen[slot]:
            raise ValueError("load_schedule: stale handle -- its staging slot has been filled again since (ring=%d)"
                             % len(self.pins))
        self.pending.extend(h["npts"])
        h["dst"].copy_(h["src"], non_blocking=True)
        ev = self.pin_events[slot]
        if ev is None:
            ev = self.pin_events[slot] = torch.cuda.Event()
        ev.record()

    def replay(self):
        """Run the next loaded step."""
        eng = self.eng
        n_pts = self.pending.pop(0)
        eng.noise_step += 1
        eng.opt_step += 1
        self.graph.replay()
        self.out, self.last = self.out1, self.last1
        eng.last = dict(self.last)
        eng.last["n_pts"] = n_pts
        if self.collective == "host":
            self._tail()
        return self.out

    def replay_all(self):
        """Run every loaded step: the run of n steps is cut greedily into the largest unrolled graphs that fit (57 = 16 + 16
        + 16 + 8 + 1) and replayed SMALLEST FIRST: launching a graph costs the host time that grows with its node count, and
        only the first launch of a run is exposed (the later ones are issued while the GPU is busy) -- so the first one
        should be the cheapest (a 20-step timed region: 4 + 16 instead of 16 + 4)."""
        eng = self.eng
        n, sizes = len(self.pending), []
        for U in self.unrolls:
            if U in self.graphs_u:
                while n >= U:
                    sizes.append(U)
                    n -= U
        sizes += [1] * n
        for U in reversed(sizes):
            if U == 1:
                self.replay()
                continue
            g, out, last = self.graphs_u[U]
            n_pts = self.pending[U - 1]
            del self.pending[:U]
            eng.noise_step += U
            eng.opt_step += U
            g.replay()
            self.out, self.last = out, last
            eng.last = dict(self.last)
            eng.last["n_pts"] = n_pts
        return self.out

    def prime(self, rounds=1):
        """Replay every captured graph `rounds` times (real training steps on block ids 0..): the first launch of a graph
        pays a one-off upload that a measurement should not hold.  For benchmarks; training does not need it.  Returns the
        number of optimiser steps run."""
        B, N = self.batch, self.eng.N_leaf
        sizes = [u for u in self.unrolls if u in self.graphs_u] + [1]
        n = 0
        for _ in range(max(int(rounds), 1)):
            for u in sizes:
                self.load_schedule([((np.arange(B) + k * B) % N, None) for k in range(u)])
                self.replay_all()
                n += u
        torch.cuda.synchronize()
        return n

    def __call__(self, idx_host, n_pts=None):
        """One step with its own one-row schedule (tests; the training loop loads an epoch at a time)."""
        self.load_schedule([(idx_host, n_pts)])
        return self.replay()


class EpochDriver:
    """The mini-batch phase of one epoch of NVFPCC.py train (NVFPCC.py:149-223) on this rank: full-size mini-batches
    replay the captured graph of their (share size, q), anything else (the short last batch, an empty share) takes the
    host-launched step.  No host synchronisation: the log line's sums stay in device accumulators
    (TrainEngine.read_epoch_stats, once per epoch)."""

    def __init__(self, eng, batch, rank=0, world=1, use_graph=True):
        from . import dist as nd
        self.eng, self.batch, self.rank, self.world, self.use_graph = eng, int(batch), rank, world, use_graph
        self.nd = nd
        self.graphs = {}
        eng.enable_epoch_stats()

    def run(self, order, q):
        eng, B = self.eng, self.batch
        n = len(order)
        nsteps = (n + B - 1) // B
        order = np.asarray(order, np.int64)
        nfull = n // B
        share = len(range(self.rank, B, self.world))     # this rank's blocks of a full mini-batch
        s = 0
        if self.use_graph and nfull > 0 and share > 0:
            # every full-size mini-batch in one go: the rows of the schedule as arrays (a Python loop over the steps costs
            # the host ~8 us each, with the GPU idle behind the epoch's read-back)
            whole = order[:nfull * B].reshape(nfull, B)
            ids_all, npts = whole[:, self.rank::self.world], eng.counts[whole].sum(axis=1).astype(np.float64)
            key = (share, q)
            g = self.graphs.get(key)
            if g is None:
                g = self.graphs[key] = GraphedTrainStep(eng, share, q)
            while s < nfull:
                e = min(nfull, s + g.CAP)
                g.load_schedule((ids_all[s:e], npts[s:e]))
                g.replay_all()
                s = e
        while s < nsteps:                                # the short last batch, empty shares, or no graph at all
            ids, whole = self.nd.shard_minibatch(order, s, B, self.rank, self.world)
            n_pts = float(eng.counts[whole].sum())
            if self.use_graph and self.world == 1 and s == nfull and len(ids) > 0:
                # one GPU: the short last mini-batch (917 mod 16 = 5 blocks) replays a single-step graph of its own size
                # instead of ~90 host launches (0.25 ms against 0.6 per epoch); same kernels, same bits
                key = (len(ids), q)
                g = self.graphs.get(key)
                if g is None:
                    g = self.graphs[key] = GraphedTrainStep(eng, len(ids), q, unroll=1)
                g.load_schedule((np.asarray(ids, np.int64)[None], np.array([n_pts])))
                g.replay_all()
            else:
                eng.train_step(ids, q, n_pts=n_pts)
            s += 1
        return nsteps
