#!/usr/bin/env python3
"""NVFPCC command line on MI355X: `train`, `encode`, `decode` with the reference's flags, defaults,
checkpoint files and pack.pk layout (/root/reference/NVFPCC.py:654-755), driven by the gfx950 step
engine (nvfpcc_amd/engine.py) instead of a DataLoader + autograd loop.

    python NVFPCC.py train longdress_vox10_1300.ply --checkpoint_dir ckpts --batchsize 16 --lambda 200 \
        --lr 1e-3 --w1 10 --w2 57 --wemb 5 --shuffle True --chanstr 8,16,8,8 --ch 3
    python NVFPCC.py encode longdress_vox10_1300.ply --batchsize 1 --chanstr 8,16,8,8 --ch 3 \
        --load_weights 0500_quantized_q4.ckpt --load_emb ckpts/0500_emb.ckpt --thh 0.65 --pack_fn pack.pk
    python NVFPCC.py decode pack.pk --batchsize 1 --chanstr 8,16,8,8 --ch 3 --thh 0.64

    python NVFPCC.py encode longdress_vox10_1300.ply ... --thh_mode count     # threshold chosen here, carried in pack.pk
    python NVFPCC.py decode pack.pk --batchsize 1 --chanstr 8,16,8,8 --ch 3   # no --thh needed then

    python NVFPCC.py train cloud.ply --from_ply ...                            # no get_octree / util_get_grids run, no .npy
    python NVFPCC.py encode cloud.ply --from_ply --pack_octree ...             # leaves travel as octree bytes; decode needs no --N
    python NVFPCC.py train cloud_vox11.ply --from_ply --bits 11 ...            # 11 or 12 bits per axis (--from_ply only)
    python NVFPCC.py encode ... --pack_lod --lod_heads ckpts/0500.ckpt         # the coarse heads travel in the pack (lod_pack)
    python NVFPCC.py decode pack.pk --lod 1 ...                                # half resolution: the trunk stops at the 16^3 head
    python NVFPCC.py encode ... --lossless                                     # the true occupancy travels too (lossless_pack)
    python NVFPCC.py decode pack.pk --lossless ...                             # rc_dec.ply holds exactly the input's voxels
    python NVFPCC.py encode ... --lossless_lod                                 # the occupancy coarse to fine (lossless_lod_pack)
    python NVFPCC.py encode ... --lossless_lod --lossless_ctx nbr              # the voxels under their parents' neighbours
    python NVFPCC.py decode pack.pk --lossless_lod 0|1|2 ...                   # exact at 32^3, 16^3 or 8^3 per block
    python NVFPCC.py encode ... --lossless_lod --lossless_ctx inter --lossless_ref prev/rc_dec.ply   # the voxels under a cloud both sides hold
    python NVFPCC.py decode pack.pk --lossless_lod 0|1|2 --lossless_ref prev/rc_dec.ply ...          # the same reference decodes it
    python NVFPCC.py encode ... --lossless_lod --lossless_ctx inter --lossless_ref prev/rc_dec.ply --lossless_mv 4   # each block under the reference moved by its own vector (lossless_mv_pack); decode needs no flag
    python NVFPCC.py train seq_%04d.ply --gof 8 --frame_start 1300 ...         # one decoder for frames 1300 .. 1307
    python NVFPCC.py encode seq_%04d.ply --gof 8 --frame_start 1300 ...        # one pack: the weights once, a frame pack each
    python NVFPCC.py decode pack.pk --frame 1303 ...                           # that frame alone; without --frame, all of them
    python NVFPCC.py train next.ply --freeze_decoder --load_weights q4.ckpt    # latents only, under a decoder that does not move
    python NVFPCC.py encode next.ply --load_weights q4.ckpt --ref_pack ref.pk  # a latents-only pack: 33 bytes name ref.pk's decoder
    python NVFPCC.py decode p.pk --ref_pack ref.pk ...                         # decoded under the reference's weights
    python NVFPCC.py train scan.ply --from_ply --voxelize [--vox_step S --vox_origin X Y Z] ...    # float coordinates, repeated points
    python NVFPCC.py encode scan.ply --from_ply --voxelize ...                 # the same flags; the lattice travels (vox_pack)
    python NVFPCC.py decode pack.pk --source_frame ...                         # also rc_dec_src.ply, in the input's frame

Additions over the reference (all optional): --device, --epochs, --seed, --ref_ply, --from_ply, --ply_format, --bits, --pack_octree, --pack_lod, --lod_heads, --lod, --lossless, --lossless_lod, --lossless_ctx, --lossless_ref, --lossless_mv, --gof, --frame_start, --frame, --freeze_decoder, --ref_pack, --thh_mode (count | block-count | d1:
nvfpcc_amd/thh_select.py picks the occupancy threshold at encode time and a `thh_pack` key carries it), --voxelize, --vox_step,
--vox_origin, --source_frame (nvfpcc_amd/voxelize.py: float clouds are voxelised on the device and a `vox_pack` key carries the lattice); multi-GPU training when launched
through torch.distributed.run (one process per GPU, leaf blocks sharded, one RCCL all-reduce per step).
Headless: no GUI window, no IPython shell.
"""
import argparse
import os
import pickle
import time
from collections import OrderedDict

import numpy as np
import torch

param_model = 'Gaussian'
prob_model = 'Gaussian'
main_loss = 'wfocal'   # distance-weighted focal loss (NVFPCC.py:27)
focal_alpha = 0.9


def _banner():
    print(f'[Info] Using {param_model} for network parameters.')
    print(f'[Info] Using {prob_model} for latent repr.')
    print(f'[Info] Using {main_loss} as main loss function, alpha={focal_alpha}')


def lr_at_epoch(base_lr, epoch):
    """Both MultiStepLR([300,400,450], 0.1) objects of the reference are bound to the DECODER optimiser
    (NVFPCC.py:117,126,253-254): x0.01 per milestone for the decoder, the latent LR never decays."""
    return base_lr * (0.01 ** sum(epoch >= m for m in (300, 400, 450)))


def _device(args):
    if not torch.cuda.is_available():
        raise RuntimeError("NVFPCC.py needs a HIP device: the NVF hot path has no CPU fallback "
                           "(the CPU oracle lives in oracle/ and is test infrastructure)")
    from nvfpcc_amd import dist as nd
    rank, local_rank, world = nd.init()
    dev = torch.device(args.device if args.device != 'cuda' else f'cuda:{local_rank}')
    torch.cuda.set_device(dev)
    return dev, rank, world


def _build_net(args, dev):
    from nvfpcc_amd import network
    from nvfpcc_amd.model import Net
    network.reset_seed()                     # SEED3.npy from the CWD if present, else the build's stand-in
    network.set_noise_seed(args.seed)
    return Net(args, param_model, args.ch, channel_str=args.chanstr).to(dev)


def _psnr1(sse, denom, peak=1023):
    with np.errstate(divide="ignore", invalid="ignore"):     # 0 / 0 prints nan, as in the reference (NVFPCC.py:259-260)
        mse1 = np.float64(sse) / np.float64(denom)
        return mse1, 20 * np.log10(peak / np.sqrt(mse1 / 3))


def _bits(args):
    """--bits of train / encode (10 when absent) after the checks that need no device: what the deeper partition does
    not reach exits here, with its reason, before any GPU work."""
    bits = getattr(args, 'bits', 10)
    if bits > 10:
        if not getattr(args, 'from_ply', False):
            raise SystemExit(f"--bits {bits} needs --from_ply: the *_l5_*.npy route (get_octree.py, util_get_grids.py) "
                             f"is 10-bit only")
        if args.ref_ply is not None:
            raise SystemExit(f"--ref_ply with --bits {bits} is not supported: the D1 / D2 metrics (nvfpcc_amd.pc_metrics) "
                             f"index a dense grid of a 1024^3 volume and stop at 10 bits per axis")
        if args.thh_mode == 'd1':
            raise SystemExit(f"--thh_mode d1 with --bits {bits} is not supported: it scores its candidates with "
                             f"nvfpcc_amd.pc_metrics, which stops at 10 bits per axis; use count or block-count")
    return bits


def _voxelize_refusals(args):
    """--voxelize / --vox_step / --vox_origin / --source_frame after the checks that need no device and no file: what
    does not fit together exits here, each with its own reason.  With --voxelize, args.vox_lattice becomes the lattice
    of --vox_step / --vox_origin (nvfpcc_amd.voxelize.Lattice), or None for the cloud's own fit."""
    from nvfpcc_amd import voxelize as vx
    cmd = args.command
    if hasattr(args, 'source_frame') and cmd != 'decode':
        raise SystemExit(f"{cmd}: --source_frame is a switch of decode: it writes the decoded cloud in the frame of the "
                         f"pack's vox_pack")
    if not hasattr(args, 'voxelize'):
        if hasattr(args, 'vox_step'):
            raise SystemExit(f"{cmd}: --vox_step {args.vox_step!r} is the lattice step of --voxelize; give --voxelize too")
        if hasattr(args, 'vox_origin'):
            raise SystemExit(f"{cmd}: --vox_origin places the lattice of --voxelize --vox_step; give both too")
        return
    if cmd == 'decode':
        raise SystemExit("decode: --voxelize belongs to train and encode; decode reads the lattice from the pack's "
                         "vox_pack (--source_frame writes the cloud in the input's frame)")
    if not hasattr(args, 'from_ply'):
        raise SystemExit(f"{cmd}: --voxelize needs --from_ply: it reads the cloud itself, with float coordinates, and "
                         f"there is no *_l5_*.npy file of such a cloud")
    args.vox_lattice = vx.lattice_from_args(args, cmd)
    if hasattr(args, 'gof') and args.vox_lattice is None:
        raise SystemExit(f"{cmd}: --gof with --voxelize needs one lattice for all frames of the group, and a fit is each "
                         f"frame's own; give --vox_step / --vox_origin")


def _load_data(args, dev, shuffle=True):
    """The dataset of `args.input`: the three `*_l5_*.npy` files next to it, or -- with --from_ply -- the cloud itself,
    pre-processed on the device (nothing is read from or written to disk besides the PLY).  -> (dataset, the
    DevicePreprocess or None)."""
    from nvfpcc_amd.dataloader import LoadedVoxelDataset

    def one(name):
        if getattr(args, 'from_ply', False):
            from nvfpcc_amd import ply_io, preprocess as pp
            if hasattr(args, 'voxelize'):   # float coordinates: the distinct lattice points stand for the cloud from here on
                from nvfpcc_amd import voxelize as vx
                try:
                    vox = vx.voxelize(ply_io.read_ply(name, coords='float')[0], dev, bits=getattr(args, 'bits', 10),
                                      lattice=args.vox_lattice)
                except (OSError, ValueError) as e:
                    raise SystemExit(f"--voxelize {name}: {e}")
                pre = pp.preprocess_device(vox.points, dev, bits=vox.lattice.bits)
                pre.vox_lattice, pre.vox_line = vox.lattice, vx.voxelize_line(vox)
                print(pre.vox_line)
            else:
                pre = pp.preprocess_device(ply_io.read_ply(name, device=dev)[0], dev, bits=getattr(args, 'bits', 10))
            return LoadedVoxelDataset.from_device(pre, shuffle=shuffle), pre
        fid = name[:-4]
        return LoadedVoxelDataset(f'{fid}_l5_origins.npy', f'{fid}_l5_gt_grid.npy', f'{fid}_l5_dist.npy',
                                  shuffle=shuffle), None
    if hasattr(args, 'gof'):    # the frames' blocks, frame-major, as one dataset; its frame(k) carries frame k's `pre`
        from nvfpcc_amd import gof
        frames, pres = zip(*[gof.quiet(one, name) for name in _gof_names(args)])
        for pre in pres:            # (quiet dropped them with the frames' [data] lines)
            if getattr(pre, 'vox_line', None):
                print(pre.vox_line)
        return gof.GofDataset(frames, shuffle=shuffle, pres=pres), None
    return one(args.input)


def _gof_names(args):
    """--gof F [--frame_start S] of train / encode: `input` is the pattern of the frames' names.  -> the F names, or None
    without --gof.  Checked by nvfpcc_amd.gof.frame_names, and so is a --ref_ply pattern: what is wrong exits here, with
    its reason, before any GPU work."""
    if not hasattr(args, 'gof'):
        if hasattr(args, 'frame_start'):
            raise SystemExit(f"--frame_start {args.frame_start} numbers the frames of --gof; give --gof too")
        return None
    from nvfpcc_amd import gof
    start = getattr(args, 'frame_start', 0)
    try:
        if args.input is None:
            raise ValueError("no input: --gof takes the pattern of the frames' names, such as seq_%04d.ply")
        names = gof.frame_names(args.input, start, args.gof, None if getattr(args, 'from_ply', False) else gof.npy_triple)
        if args.ref_ply is not None:
            gof.frame_names(args.ref_ply, start, args.gof)
    except ValueError as e:
        raise SystemExit(f"--gof {args.gof}: {e}")
    return names


def _load_ref_pack(args, what):
    """--ref_pack: the reference pack, which must carry a decoder of its own."""
    try:
        with open(args.ref_pack, 'rb') as f:
            ref = pickle.load(f)
    except (OSError, pickle.UnpicklingError, EOFError) as e:
        raise SystemExit(f"{what} --ref_pack {args.ref_pack}: {e}")
    if not isinstance(ref, dict) or 'net_weight_pack' not in ref:
        raise SystemExit(f"{what} --ref_pack {args.ref_pack}: it holds no net_weight_pack (a latents-only pack cannot be "
                         f"a reference)")
    return ref


def fit_frozen(args):
    """train --freeze_decoder: the latents of the input's blocks fitted under the decoder of --load_weights, which
    does not move (TrainEngine.fit_latents; --epochs is the number of latent steps).  One [Fit] line per evaluation;
    the table goes to <checkpoint_dir>/%04d_emb.ckpt under the number of the last step, counted from 0 as train counts
    its epochs."""
    from nvfpcc_amd import pframe
    from nvfpcc_amd.engine import TrainEngine
    if not args.load_weights:
        raise SystemExit("train --freeze_decoder: no decoder to freeze; name the quantised checkpoint with --load_weights")
    warm = hasattr(args, 'ref_pack')
    if warm != bool(args.load_emb):
        raise SystemExit("train --freeze_decoder: --ref_pack and --load_emb warm-start the table together (the reference's "
                         "pack gives its blocks' origins, --load_emb their rows); give both or neither")
    if args.epochs < 1:
        raise SystemExit(f"train --freeze_decoder: --epochs {args.epochs} is the number of latent steps, at least 1")
    _bits(args)
    _gof_names(args)
    ref = _load_ref_pack(args, 'train --freeze_decoder') if warm else None
    dev, rank, world = _device(args)
    if world > 1:
        raise SystemExit("train --freeze_decoder runs on one GPU: the blocks of a frame are one pass")
    data, _ = _load_data(args, dev, shuffle=False)
    print('Using lambda: ', args.lmbda)
    net = _build_net(args, dev)
    d = torch.load(args.load_weights, map_location=dev)
    net.load_state_dict({k: v for k, v in d.items() if 'init_coords' not in k}, strict=False)
    emb = None
    if warm:
        ref_emb = torch.load(args.load_emb, map_location='cpu').float()
        origins = np.array([data.origins[i] for i in range(len(data))], dtype=np.int64)
        try:
            emb = pframe.warm_start(ref_emb, pframe.pack_origins(ref), origins)
        except ValueError as e:
            raise SystemExit(f"train --freeze_decoder: {args.load_emb} / {args.ref_pack}: {e}")
    gt, dist = data.to_device(dev)
    eng = TrainEngine(net, gt, dist, n_points_total=float(data.N), lmbda=args.lmbda, w1=args.w1, w2=args.w2,
                      lr=args.lr, wemb=args.wemb, emb=emb, seed=args.seed)
    print('Embedding learning rate: %f x %f = %f' % (args.lr, args.wemb, args.lr * args.wemb))
    t0, n_pts = time.time(), float(data.N)

    def report(step, J, improved, bits):
        torch.cuda.synchronize()
        print(FIT_LINE % (step, time.time() - t0, J.sum().item(), int(improved.sum().item()), data.N_leaf,
                          bits.sum().item() / n_pts))
    eng.fit_latents(args.epochs, eval_every=10, report=report)
    print('[INFO] Saving')
    os.makedirs(args.checkpoint_dir, exist_ok=True)
    torch.save(eng.emb.detach().clone(), './%s/%04d_emb.ckpt' % (args.checkpoint_dir, args.epochs - 1))


FIT_LINE = '[Fit %04d %.1f seconds] J: %.9e improved: %d / %d b_latent: %.4f'


def train(args):
    from nvfpcc_amd import dist as nd, ops
    from nvfpcc_amd.engine import TrainEngine, EpochDriver
    _voxelize_refusals(args)
    if hasattr(args, 'freeze_decoder'):
        return fit_frozen(args)
    peak = (1 << _bits(args)) - 1
    _gof_names(args)
    dev, rank, world = _device(args)
    say = print if rank == 0 else (lambda *a, **k: None)
    say(f'Rate loss = {args.w1} * b1 + b2 + {args.w2} * b3')
    data, _ = _load_data(args, dev)
    say('Using lambda: ', args.lmbda)
    net = _build_net(args, dev)
    gt, dist = data.to_device(dev)
    eng = TrainEngine(net, gt, dist, n_points_total=float(data.N), lmbda=args.lmbda, w1=args.w1, w2=args.w2,
                      lr=args.lr, wemb=args.wemb, seed=args.seed)
    nd.attach(eng, world)
    say('Embedding learning rate: %f x %f = %f' % (args.lr, args.wemb, args.lr * args.wemb))
    B, N = args.batchsize, data.N_leaf
    lo, hi = nd.shard_range(N, rank, world)
    # mini-batch phase: full-size mini-batches replay one captured HIP graph per (share, q); the log line's sums
    # live in device accumulators and are read ONCE per epoch (the reference syncs ~14 .item()s per step)
    driver = EpochDriver(eng, B, rank, world, use_graph=os.environ.get("NVF_TRAIN_GRAPH", "1") != "0")
    q = 1
    for epoch in range(0, args.epochs):
        t0 = time.time()
        if epoch == args.phase_change:
            q = 2
        eng.lr = lr_at_epoch(args.lr, epoch)
        order = data.epoch_order(epoch, bool(args.shuffle), seed=args.seed)
        nsteps = driver.run(order, q)
        # latent update on this rank's shard (every rank advances the noise counter), then re-synchronise the table
        if hi > lo:
            eng.latent_step_chunked(q, lo, hi)      # (a group of frames can hold more blocks than one pass should)
        else:
            eng.noise_step += 1
        nd.allgather_rows_(eng.emb, rank, world)
        # NaN guards of NVFPCC.py:199-212 are checked here, on the summed counters (raises ValueError)
        acc = eng.read_epoch_stats(reduce=nd.allreduce_sum_ if world > 1 else None, world=world)
        say(TRAIN_LINE % ((epoch, time.time() - t0) + tuple(eng.train_log_fields(acc, nsteps, peak=peak))))
        if epoch % 10 == 0:
            if rank == 0:
                print('[INFO] Saving')
                os.makedirs(args.checkpoint_dir, exist_ok=True)
                sd = OrderedDict((k, v.detach().clone()) for k, v in net.state_dict().items())
                torch.save(sd, './%s/%04d.ckpt' % (args.checkpoint_dir, epoch))
                torch.save(eng.emb.detach().clone(), './%s/%04d_emb.ckpt' % (args.checkpoint_dir, epoch))
            # the every-10th-epoch evaluation (NVFPCC.py:308-392), sharded: each rank its contiguous blocks, one small
            # all-reduce of the 22 log sums (the reference runs it on its single device)
            t1 = time.time()
            fields = tuple(test_log_fields(eng, net, data.N, args.lmbda, rank, world, nd.allreduce_sum_, peak=peak))
            say(TEST_LINE % ((epoch, time.time() - t1) + fields))


def test_log_fields(eng, net, n_points, lmbda, rank=0, world=1, reduce=None, peak=1023):
    """The 17 numbers of the reference's TEST line (NVFPCC.py:308-392): full-batch net(emb, 'eval', 2), the same
    losses / metrics as the TRAIN line on ALL blocks (one "mini-batch": cnt = 1), and b_all = (latent bits + network
    bits incl. the side information of Net.get_network_bits) / N.  Quirk kept: its Loss adds lambda * (b_latent + b_net)
    without the w1 / w2 weights (:347).
    Data parallelism: every rank evaluates its contiguous shard of the blocks (dist.shard_range) and ONE all-reduce of
    the 22 additive sums (`reduce`) gives every rank the full-batch numbers -- call it on every rank."""
    from nvfpcc_amd import dist as nd
    lo, hi = nd.shard_range(eng.N_leaf, rank, world)
    sums = eng.eval_sums(lo, hi, q=2)
    if reduce is not None and world > 1:
        reduce(sums)
    return test_fields_from_sums(sums.double().cpu().numpy(), eng.weight_bits(), float(eng.counts.sum()), float(n_points),
                                 lmbda, net.get_network_bits(), peak=peak)


def test_fields_from_sums(sums, weight_bits, n_pts, n_points, lmbda, network_bits, peak=1023):
    """Host arithmetic of the TEST line from the 22 additive sums of TrainEngine.eval_sums (focal terms [0:3], metric
    counts [3:21], latent bits [21]).  peak: 2^bits - 1 of the cloud, the peak of PSNR1."""
    ls, c, lat_bits = sums[0:3], sums[3:21], float(sums[21])
    b_latent, b_net = lat_bits / n_pts, float(weight_bits) / float(n_points)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = [c[6 * t + k] / c[6 * t + k + 1] for t in range(3) for k in (0, 2)]
        mse1 = c[4] / c[5]
        psnr1 = 20 * np.log10(peak / np.sqrt(mse1 / 3))
    b_all = (lat_bits + network_bits) / float(n_points)
    return [ls[0] + ls[1] + ls[2] + lmbda * (b_latent + b_net), 0.0, 0.0, r[0], r[1], ls[1], ls[2], r[2], r[3], r[4],
            r[5], b_latent + b_net, b_latent, b_net, b_all, mse1, psnr1]


# the reference's format strings (NVFPCC.py:261, 371), character for character: anything that parses its log parses ours
TRAIN_LINE = ('[Epoch %04d TRAIN %.1f seconds] Loss: %.4e PosiPenal: %.4f PosiGain: %.4f Pacc: %.4f Nacc: %.4f '
              'S1 Loss: %.4f S2 Loss: %.4f S1Pacc: %.4f S1Nacc: %.4f S2Pacc: %.4f S2Nacc: %.4f bpp: %.4f '
              'b_latent: %.4f  b_net: %.4f MSE1: %.4f PSNR1: %.4f')
TEST_LINE = ('[Epoch %04d TEST %.1f seconds] Loss: %.4e PosiPenal: %.4f PosiGain: %.4f Pacc: %.4f Nacc: %.4f '
             'S1 Loss: %.4f S2 Loss: %.4f S1Pacc: %.4f S1Nacc: %.4f S2Pacc: %.4f S2Nacc: %.4f bpp: %.4f '
             'b_latent: %.4f b_net: %.4f b_all: %.4f MSE1: %.4f PSNR1: %.4f')


def encode(args):
    """Pack everything the decoder needs (NVFPCC.py:395-554)."""
    from nvfpcc_amd import weight_codec
    _voxelize_refusals(args)
    lossless_ctx_refusals(args)
    bits = _bits(args)
    names = _gof_names(args)
    fmt = getattr(args, 'ply_format', 'ascii')
    dev, rank, world = _device(args)
    data, pre = _load_data(args, dev, shuffle=False)
    net = _build_net(args, dev)
    net_weight_pack = weight_codec.enc_dec_from_file(args.load_weights, qp=int(args.qp))
    as_p = hasattr(args, 'ref_pack')
    if as_p:    # a latents-only pack: the decoder of --load_weights must be the reference's, byte for byte
        from nvfpcc_amd import pframe
        ref = _load_ref_pack(args, 'encode')
        if pframe.digest(net_weight_pack) != pframe.digest(ref['net_weight_pack']):
            raise SystemExit(f"encode --ref_pack: the decoder of {args.load_weights} (at --qp {args.qp:g}) is not the one "
                             f"{args.ref_pack} carries; a latents-only pack is coded under its reference's decoder")
    d = torch.load(args.load_weights, map_location=dev)
    net.load_state_dict({k: v for k, v in d.items() if 'init_coords' not in k}, strict=False)
    emb = torch.load(args.load_emb, map_location=dev).to(dev).float().contiguous()
    if names is not None:
        return _encode_gof(args, net, net_weight_pack, emb, data, dev, bits, fmt, as_p)

    def write(frame_pack):
        total_pack = {'net_weight_pack': net_weight_pack, **frame_pack}
        with open(args.pack_fn, 'wb') as f:
            pickle.dump(pframe.split(total_pack) if as_p else total_pack, f)
    _encode_frame(args, net, net_weight_pack, emb, data, pre, dev, bits, fmt, 'rc_enc', write,
                  decoder_bits=8 * pframe.REF_PACK_BYTES if as_p else None)


def _encode_gof(args, net, net_weight_pack, emb, data, dev, bits, fmt, as_p=False):
    """encode --gof: every frame through _encode_frame with its rows of --load_emb, into one pack
    (nvfpcc_amd.gof: the weights once, gof_pack, a frame pack each).  as_p: written as a latents-only pack
    (nvfpcc_amd.pframe.split), whose closing lines count ref_pack in place of the weights."""
    import contextlib
    import io
    from nvfpcc_amd import gof
    start = getattr(args, 'frame_start', 0)
    if emb.shape[0] != data.N_leaf:
        raise SystemExit(f"encode --gof {args.gof}: {args.load_emb} holds {emb.shape[0]} rows, the group's frames "
                         f"{data.N_leaf} leaf blocks")
    frames = []
    for k in range(len(data.frame_points)):
        number = start + k
        lo, hi = int(data.frame_ranges[k]), int(data.frame_ranges[k + 1])
        fargs = argparse.Namespace(**vars(args))
        fargs.ref_ply = None if args.ref_ply is None else args.ref_ply % number
        lines = io.StringIO()       # the frame's lines follow its [Frame] line, whose numbers they come before
        try:
            with contextlib.redirect_stdout(lines):
                view = data.frame(k)
                frame_pack, report = _encode_frame(fargs, net, net_weight_pack, emb[lo:hi].contiguous(), view, view.pre, dev,
                                                   bits, fmt, 'rc_enc_%04d' % number, None)
        except BaseException:
            print(lines.getvalue(), end='')
            raise
        print(gof.frame_line(number, report['points'], report['blocks'], report['latent_bits'], report['side_bits']))
        print(lines.getvalue(), end='')
        frames.append(frame_pack)
    total_pack = {'net_weight_pack': net_weight_pack,
                  'gof_pack': gof.write_gof_pack(start, np.diff(data.frame_ranges), data.frame_points), 'frames': frames}
    if as_p:
        from nvfpcc_amd import pframe
        total_pack = pframe.split(total_pack)
    with open(args.pack_fn, 'wb') as f:
        pickle.dump(total_pack, f)
    for line in gof.gof_lines(total_pack):
        print(line)


def _encode_frame(args, net, net_weight_pack, emb, data, pre, dev, bits, fmt, stem, write_pack, decoder_bits=None):
    """Code one frame: the latents `emb` of its blocks under `net` (whose bytes are `net_weight_pack`), the side packs
    the flags ask for, and its reconstruction into `stem`.ply (and `stem`_lod1.ply / _lod2.ply).  write_pack(frame_pack)
    is called as soon as the pack is complete, before the reconstruction; None: the frame belongs to a group, nothing
    is written and its Gross bpp line is the group's.  decoder_bits: what the written pack pays for its decoder when that
    is not the weights' stream (a latents-only pack: its ref_pack).  -> (frame_pack: the plain pack without net_weight_pack, report:
    {'points', 'blocks', 'latent_bits', 'side_bits'})."""
    from nvfpcc_amd import ops, latent_codec
    from nvfpcc_amd import ply_io
    from nvfpcc_amd.recon import eval_batches, reconstruct_points
    net_bits = len(net_weight_pack['bit_stream']) * 8 if decoder_bits is None else int(decoder_bits)
    np_origins = np.array([data.origins[i] for i in range(len(data))], dtype=np.int16)
    with torch.no_grad():
        info = net.get_latent_code(emb)
    print('Estimated bit rate: ', info['latent_likelihood'].sum())
    latent_pack = latent_codec.arithmetic_enc(info['quantized_latent'], info['sigma'], info['mu'])
    if getattr(args, 'pack_octree', False):                  # the partition as octree bytes instead of 6 raw bytes per leaf
        from nvfpcc_amd import preprocess as pp
        octree_pack = pre.octree_pack() if pre is not None else pp.octree_pack_from_origins(np_origins)
        total_pack = {'net_weight_pack': net_weight_pack, 'latent_pack': latent_pack, 'octree_pack': octree_pack}
    else:
        total_pack = {'net_weight_pack': net_weight_pack, 'origins': np_origins, 'latent_pack': latent_pack}
    batch = max(int(args.batchsize), 1)
    thh, sel = args.thh, None
    if args.thh_mode not in (None, 'fixed'):
        sel = _select_threshold(args.thh_mode, net, info['quantized_latent'].detach(), data, np_origins, dev, batch)
        thh = sel['t']
        total_pack['thh_pack'] = sel['pack']
    lod = None
    if getattr(args, 'pack_lod', False):    # the two coarse heads and their thresholds travel too: decode --lod 1 | 2
        lod = _encode_lod(args, net, info['quantized_latent'].detach(), data, np_origins, dev, batch)
        total_pack['lod_pack'] = lod['pack']
    lossless = None
    if getattr(args, 'lossless', False):    # the true occupancy, coded under the field the pack's own bytes decode to
        lossless = _encode_lossless(args, total_pack, data, dev, batch)
        total_pack['lossless_pack'] = lossless['pack']
    lossless_lod = None
    if getattr(args, 'lossless_lod', None) is not None:     # the same occupancy coarse to fine: exact at 8^3, 16^3, 32^3
        lossless_lod = _encode_lossless_lod(args, total_pack, data, dev, batch)
        total_pack['lossless_lod_pack'] = lossless_lod['pack']
        if 'mv_pack' in lossless_lod:       # --lossless_mv: the vectors the reference words were fetched under
            total_pack['lossless_mv_pack'] = lossless_lod['mv_pack']
    lattice = getattr(pre, 'vox_lattice', None)
    if lattice is not None:                 # --voxelize: the lattice the points lie on, for decode --source_frame
        from nvfpcc_amd import voxelize as vx
        total_pack['vox_pack'] = vx.pack(lattice)
    frame_pack = {k: v for k, v in total_pack.items() if k != 'net_weight_pack'}
    if write_pack is not None:
        write_pack(frame_pack)
    print('Start to reconstruct')
    pts, counts = reconstruct_points(net, info['quantized_latent'].detach(), np_origins, thh, batch=batch)
    gt, dist = data.to_device(dev)
    with torch.no_grad():
        out = torch.cat([o for _, _, o in eval_batches(net, info['quantized_latent'], 64)], 0)
    if isinstance(thh, torch.Tensor):       # one threshold per block: the six sums block by block
        m = torch.zeros(6, device=dev)
        for b, t in enumerate(thh.tolist()):
            ops.metrics(out[b:b + 1], gt[b:b + 1], dist[b:b + 1], t, t, out=m, accumulate=True)
        m = m.cpu().numpy()
    else:
        m = ops.metrics(out, gt, dist, thh, thh).cpu().numpy()
    latent_bits = len(latent_pack['latent_byte_stream']) * 8
    side_bits = (0 if sel is None else 8 * len(sel['pack'])) + 8 * len(total_pack.get('octree_pack', b''))
    side_bits += 8 * len(total_pack.get('lod_pack', b'')) + 8 * len(total_pack.get('lossless_pack', b''))
    side_bits += 8 * len(total_pack.get('lossless_lod_pack', b'')) + 8 * len(total_pack.get('lossless_mv_pack', b''))
    side_bits += 8 * len(total_pack.get('vox_pack', b''))
    if sel is not None:
        print(sel['line'])
    if write_pack is not None:
        print('[Latent code] Gross bpp: %.4f' % ((latent_bits + net_bits + side_bits) / data.N))
    print('[Recon] Pacc: %.4f Nacc: %.4f MSE1: %.4f PSNR1: %.4f' % (
        m[0] / max(m[1], 1), m[2] / max(m[3], 1), *_psnr1(m[4], m[5], (1 << bits) - 1)))
    ply_io.write_ply(stem + '.ply', pts, fmt=fmt, device=dev)
    _print_pc_error(args, pts, dev, lattice=lattice)
    if lod is not None:
        for level, (line, lod_pts) in enumerate(zip(lod['lines'], lod['points']), 1):
            print(line)
            ply_io.write_ply(stem + '_lod%d.ply' % level, lod_pts, fmt=fmt, device=dev)
    if lossless is not None:
        print(lossless['line'])
    if lossless_lod is not None:
        print(lossless_lod['line'])
    return frame_pack, {'points': int(data.N), 'blocks': int(data.N_leaf), 'latent_bits': latent_bits, 'side_bits': side_bits}


def _encode_lossless(args, total_pack, data, dev, batch):
    """encode --lossless: the decoder exactly as decode() rebuilds it from the pack's bytes (_decoder_from_pack), the
    occupancy of every leaf block coded under its probabilities (nvfpcc_amd.lossless_pack), and the stream decoded again
    on the device: a pack whose words differ from the input's occupancy is not written.
    -> {'pack': lossless_pack bytes, 'line': the [Lossless] line}."""
    import contextlib
    import io
    from nvfpcc_amd import lossless_pack as lp
    with contextlib.redirect_stdout(io.StringIO()):     # the decoder's own progress lines belong to decode
        net, latents = _decoder_from_pack(args, total_pack, dev)
    latents = latents[:data.N_leaf].contiguous()
    gt, _ = data.to_device(dev)
    try:
        pack, info = lp.encode_occupancy(net, latents, gt, batch=batch, group=lp.GROUP)
        words, counts = lp.decode_occupancy(net, latents, pack, batch=batch)
    except ValueError as e:
        raise SystemExit(f"encode --lossless: {e}")
    if not torch.equal(words, info['gt_words']) or int(counts.sum().item()) != int(data.N):
        raise SystemExit("encode --lossless: the stream does not decode to the input's occupancy; no pack written")
    return {'pack': pack, 'line': lp.lossless_line(len(pack), data.N, info['ideal_bits'], lp.GROUP)}


def _encode_lossless_lod(args, total_pack, data, dev, batch):
    """encode --lossless_lod: as _encode_lossless, with the coarse-to-fine coder (nvfpcc_amd.lossless_lod_pack).  The
    stream is decoded again at all three levels: a pack that does not reproduce the input's occupancy and its two
    max-pools is not written.  --lossless_ctx nbr: the voxels under their parents' neighbours
    (nvfpcc_amd.lossless_nbr_pack), the same key.  --lossless_ctx inter: under the cloud of --lossless_ref as well
    (nvfpcc_amd.lossless_inter_pack), rasterised onto this frame's blocks; the same key again.  --lossless_mv R: the
    reference words are fetched block by block under the vectors of a search of radius R (nvfpcc_amd.lossless_mv_pack);
    the coder sees only those words.
    -> {'pack': lossless_lod_pack bytes, 'line': the [LosslessLoD] lines, 'mv_pack': lossless_mv_pack bytes with
    --lossless_mv}."""
    import contextlib
    import io
    ctx = getattr(args, 'lossless_ctx', 'field')
    if ctx == 'inter':
        from nvfpcc_amd import lossless_inter_pack as lp
    elif ctx == 'nbr':
        from nvfpcc_amd import lossless_nbr_pack as lp
    else:
        from nvfpcc_amd import lossless_lod_pack as lp
    with contextlib.redirect_stdout(io.StringIO()):     # the decoder's own progress lines belong to decode
        net, latents = _decoder_from_pack(args, total_pack, dev)
    latents = latents[:data.N_leaf].contiguous()
    gt, _ = data.to_device(dev)
    ref, ref_line, mv_pack = (), None, None
    if ctx == 'inter':
        ref, ref_line, mv_pack = _lossless_reference(args.lossless_ref, np.array([data.origins[i] for i in range(len(data))]),
                                                     dev, search=(gt, args.lossless_mv) if hasattr(args, 'lossless_mv') else None)
    try:
        pack, info = lp.encode_occupancy(net, latents, gt, *ref, batch=batch, group=lp.GROUP)
        for level in (2, 1, 0):
            words, counts = lp.decode_occupancy(net, latents, pack, *ref, level=level, batch=batch)
            if not torch.equal(words, info['gt_words'][level]) or (level == 0 and int(counts.sum().item()) != int(data.N)):
                raise SystemExit(f"encode --lossless_lod: the stream does not decode to the input's occupancy at level "
                                 f"{level}; no pack written")
    except ValueError as e:
        raise SystemExit(f"encode --lossless_lod: {e}")
    line = lp.lossless_lod_line(len(pack), data.N, info['ideal_bits'], info['contexts'], info['symbols'], lp.GROUP)
    out = {'pack': pack, 'line': line if ref_line is None else line + '\n' + ref_line}
    if mv_pack is not None:
        out['mv_pack'] = mv_pack
    return out


def _lossless_reference(fn, origins, dev, search=None, mv_pack=None):
    """--lossless_ref: the cloud of `fn` (ASCII or binary PLY) rasterised onto the blocks at `origins`
    -> ((the reference words on the device,), the [LosslessLoD] lines that say what was read, the lossless_mv_pack bytes
    or None).  search = (gt float [N, 32768] on the device, radius): encode --lossless_mv, the vectors are searched and
    packed; mv_pack: the bytes a pack carries, decode.  Either way the words are fetched under the vectors."""
    from nvfpcc_amd import lossless_inter_pack, lossless_mv_pack, ply_io
    try:
        pts = np.asarray(ply_io.read_ply(fn)[0])
    except (OSError, ValueError) as e:
        raise SystemExit(f"--lossless_ref {fn}: {e}")
    pts, origins = np.rint(pts).astype(np.int64), np.asarray(origins, np.int64)
    if search is None and mv_pack is None:
        words, dropped = lossless_inter_pack.reference_words(pts, origins, dev)
        return (words,), '[LosslessLoD] reference: %s points: %d dropped: %d' % (fn, pts.shape[0], dropped), None
    own = lossless_mv_pack.reference_blocks(pts, dev)
    if search is not None:
        gt, radius = search
        mv = lossless_mv_pack.search(lossless_mv_pack.frame_words(gt), own, origins, radius)[0].cpu().numpy()
        mv_pack = lossless_mv_pack.write(radius, mv)
    else:
        info = lossless_mv_pack.read(mv_pack, origins.shape[0])
        mv, radius = info['mv'], info['radius']
    words = lossless_mv_pack.compensated_words(own, origins, mv)
    lines = '[LosslessLoD] reference: %s points: %d blocks: %d\n' % (fn, pts.shape[0], own[1].shape[0]) + \
        lossless_mv_pack.mv_line(radius, mv, len(mv_pack))
    return (words,), lines, mv_pack


def _encode_lod(args, net, latents, data, origins, dev, batch):
    """encode --pack_lod: the coarse heads (conv1_cls = level 1, conv0_cls = level 2) rounded to float16 in `net`, the
    threshold of each level chosen by count against the max-pooled ground truth, and the level's cloud through
    ops.head_points.  -> {'pack': lod_pack bytes, 'lines': the two [LoD l] lines, 'points': the two clouds}."""
    from nvfpcc_amd import lod_pack as lp, ops, thh_select as ts
    from nvfpcc_amd.recon import eval_batches, reconstruct_points_lod
    src = getattr(args, 'lod_heads', None) or args.load_weights
    try:
        heads = lp.head_tensors(torch.load(src, map_location='cpu'))
    except KeyError as e:
        raise SystemExit(f"encode --pack_lod: {src} holds no {e.args[0]} (manipulate_weights.py drops the coarse heads); "
                         f"name the checkpoint that training wrote with --lod_heads")
    c1, c2 = lp.head_channels(args.chanstr)
    if heads[lp.HEAD_KEYS[0]].shape != (1, c1, 3, 3, 3) or heads[lp.HEAD_KEYS[2]].shape != (1, c2, 3, 3, 3):
        raise SystemExit(f"encode --pack_lod: the coarse heads of {src} do not fit --chanstr {args.chanstr}")
    net.load_state_dict(heads, strict=False)
    rounded = lp.round_heads_(net)          # before anything is evaluated at a coarse level: the decoder's numbers
    g, _ = data.to_device(dev)
    out = {'t': [], 'lines': [], 'points': []}
    for level in (1, 2):
        g = ops.maxpool2(g.contiguous())
        k = int((g != 0).sum().item())      # occupied coarse voxels of the input
        with torch.no_grad():
            p = torch.cat([o[1] for _, _, o in eval_batches(net, latents, batch, level, return_p=True)], 0)
        t = float(ts.threshold_for_count(p, k).item())
        m = ops.metrics(p, g, None, t, t).cpu().numpy()
        pts, _ = reconstruct_points_lod(net, latents, origins, level, t, batch=batch)
        out['t'].append(t)
        out['lines'].append(lp.lod_line(level, t, pts.shape[0], m[0] / max(m[1], 1), m[2] / max(m[3], 1)))
        out['points'].append(pts)
    out['pack'] = lp.write_lod_pack(out['t'][0], out['t'][1], *[rounded[k] for k in lp.HEAD_KEYS])
    return out


def _select_threshold(mode, net, latents, data, origins, dev, batch):
    """--thh_mode count | block-count | d1 at the encoder: the eval forward of every block stays resident and
    nvfpcc_amd.thh_select picks the threshold(s).  -> {'t': float | tensor [N_leaf], 'pack': bytes, 'line': str}."""
    from nvfpcc_amd import thh_select as ts
    from nvfpcc_amd.recon import eval_batches
    ts.check_resident(latents.shape[0])
    with torch.no_grad():
        p_all = torch.cat([o for _, _, o in eval_batches(net, latents, batch)], 0)
    k_b = data.gt_grid.reshape(data.N_leaf, -1).astype(bool).sum(1)
    if mode == 'block-count':
        sel = ts.choose(mode, p_all, block_counts=k_b)
    elif mode == 'count':
        sel = ts.choose(mode, p_all, n_points=int(data.N))
    else:
        gt8 = torch.from_numpy(np.ascontiguousarray(data.gt_grid != 0).astype(np.uint8)).to(dev)
        sel = ts.choose(mode, p_all, origins=origins, n_points=int(data.N), gt=gt8,
                        d2=ts.d2_from_dist(data.dist).to(dev).contiguous())
    if sel['note']:
        print('[Threshold] ' + sel['note'])
    decided, t = sel['mode'], sel['t']
    if decided == 'block-count':
        return {'t': t, 'pack': ts.write_thh_pack(decided, block_counts=k_b),
                'line': ts.threshold_line(decided, block_counts=k_b, thresholds=t.cpu().numpy())}
    return {'t': t, 'pack': ts.write_thh_pack(decided, t=t), 'line': ts.threshold_line(decided, t=t)}


def decode(args):
    """Decode from a pack (NVFPCC.py:557-652)."""
    if hasattr(args, 'lossless_mv'):
        raise SystemExit(f"decode: --lossless_mv {args.lossless_mv} is the search radius of encode; decode reads the "
                         f"vectors from the pack's lossless_mv_pack")
    _voxelize_refusals(args)
    lossless_refusals(args, None)
    lossless_lod_refusals(args, None)
    fmt = getattr(args, 'ply_format', 'ascii')
    dev, rank, world = _device(args)
    net = _build_net(args, torch.device('cpu'))
    with open(args.input, 'rb') as f:
        total_pack = pickle.load(f)
    if 'ref_pack' in total_pack:            # a latents-only pack: its decoder is the reference's (nvfpcc_amd.pframe)
        from nvfpcc_amd import pframe
        if not hasattr(args, 'ref_pack'):
            raise SystemExit(f"decode {args.input}: a latents-only pack, coded under another pack's decoder; name that "
                             f"pack with --ref_pack")
        try:
            total_pack = pframe.join(total_pack, _load_ref_pack(args, 'decode'))
        except ValueError as e:
            raise SystemExit(f"decode {args.input} --ref_pack {args.ref_pack}: {e}")
    elif hasattr(args, 'ref_pack'):
        print(f'[Info] {args.input} carries its own decoder; --ref_pack {args.ref_pack} is not read')
    if 'gof_pack' in total_pack:            # a group of frames: --frame K alone, or every frame
        return _decode_gof(args, total_pack, dev, fmt, net)
    if hasattr(args, 'frame'):
        raise SystemExit(f"decode --frame {args.frame}: {args.input} carries no gof_pack (it holds one cloud, encoded "
                         f"without --gof)")
    _decode_pack(args, total_pack, dev, fmt, net, 'rc_dec.ply')


def _decode_gof(args, total_pack, dev, fmt, net):
    """decode of a group (nvfpcc_amd.gof): frame K - start with --frame K into rc_dec.ply, else every frame into
    rc_dec_%04d.ply, each as the plain pack gof.extract makes of it -- nothing of another frame is read or run.  --N is
    ignored: a frame's own origins or octree give its count.  A frame that cannot be decoded is named; the others of a
    whole-group decode are still written and the exit status is non-zero."""
    from nvfpcc_amd import gof
    try:
        info = gof.read_gof_pack(total_pack['gof_pack'])
        start, F = info['start'], len(info['n_leaf'])
        if hasattr(args, 'frame'):
            if not start <= args.frame < start + F:
                raise ValueError(f"--frame {args.frame} is outside the group's frames {start} .. {start + F - 1}")
            numbers = [args.frame]
        else:
            numbers = list(range(start, start + F))
            if args.ref_ply is not None:
                gof.frame_names(args.ref_ply, start, F)
    except ValueError as e:
        raise SystemExit(f"decode {args.input}: {e}")
    failed = []
    for number in numbers:
        fargs = argparse.Namespace(**vars(args))
        try:
            pack = gof.extract(total_pack, number - start)
            fargs.N = gof.frame_leaves(pack)
            if args.ref_ply is not None and not hasattr(args, 'frame'):
                fargs.ref_ply = args.ref_ply % number
            if len(numbers) > 1:
                print('[Frame %04d]' % number)
            _decode_pack(fargs, pack, dev, fmt, net, 'rc_dec.ply' if hasattr(args, 'frame') else 'rc_dec_%04d.ply' % number)
        except (SystemExit, ValueError, RuntimeError, IndexError, KeyError, EOFError) as e:
            if hasattr(args, 'frame'):
                raise SystemExit(f"decode {args.input}: frame {number:04d}: {e}")
            failed.append('%04d' % number)
            print(f"decode {args.input}: frame {number:04d}: {e}")
        net = None                          # the next frame gets a decoder of its own
    if failed:
        raise SystemExit(f"decode {args.input}: {len(failed)} of {F} frames could not be decoded: {' '.join(failed)}")


def _decode_pack(args, total_pack, dev, fmt, net, out_fn):
    """One plain pack into the cloud `out_fn`.  net: a fresh Net on the host, or None to build one."""
    from nvfpcc_amd import ply_io
    from nvfpcc_amd.recon import reconstruct_points, reconstruct_points_lod
    lossless_refusals(args, total_pack)
    lossless_lod_refusals(args, total_pack)
    lattice = None
    if 'vox_pack' in total_pack:            # read only for --source_frame and --ref_ply; the decoded cloud does not depend on it
        from nvfpcc_amd import voxelize as vx
        try:
            lattice = vx.unpack(total_pack['vox_pack'])
        except ValueError as e:
            raise SystemExit(f"decode {args.input}: {e}")
    elif hasattr(args, 'source_frame'):
        raise SystemExit(f"decode --source_frame: {args.input} carries no vox_pack (it was encoded without --voxelize): its "
                         f"cloud has no other frame than the lattice")
    lod, lod_side = getattr(args, 'lod', 0), None
    if lod:
        from nvfpcc_amd import lod_pack as lp
        if 'lod_pack' not in total_pack:
            raise SystemExit(f"decode --lod {lod}: {args.input} carries no lod_pack (it was encoded without --pack_lod)")
        try:
            lod_side = lp.read_lod_pack(total_pack['lod_pack'], args.chanstr)
        except ValueError as e:
            raise SystemExit(f"decode --lod {lod}: {e}")
    net, latents = _decoder_from_pack(args, total_pack, dev, net, lod_side)
    if 'octree_pack' in total_pack:         # the leaves and their count come from the pack, not from --N
        from nvfpcc_amd.preprocess import read_octree_pack
        origins = read_octree_pack(total_pack['octree_pack']).astype(np.int16)
        n = origins.shape[0]
    else:
        n = int(args.N)
        origins = total_pack['origins'][:n]
    print('Start to reconstruct')
    latents, batch, level = latents[:n].contiguous(), max(int(args.batchsize), 1), 0
    if getattr(args, 'lossless', False):    # the input's own voxels: the occupancy words decoded under the field
        from nvfpcc_amd import lossless_pack as lp
        try:
            words, counts = lp.decode_occupancy(net, latents, total_pack['lossless_pack'], batch=batch)
        except ValueError as e:
            raise SystemExit(f"decode --lossless: {e}")
        pts = lp.points_from_words(words, counts, origins)
        print('[Lossless] points: %d' % pts.shape[0])
    elif getattr(args, 'lossless_lod', None) is not None:   # the input's voxels, or their exact 2^3 / 4^3 max-pool
        from nvfpcc_amd import lossless_inter_pack
        level = int(args.lossless_lod)
        try:
            llp = lossless_inter_pack.module_of(total_pack['lossless_lod_pack'])   # byte 0: which contexts coded it
            ref = ()
            if llp is lossless_inter_pack:
                if not hasattr(args, 'lossless_ref'):
                    raise SystemExit(f"decode --lossless_lod {level}: the lossless_lod_pack of {args.input} was coded under "
                                     f"a reference cloud (--lossless_ctx inter); name that cloud with --lossless_ref")
                ref, ref_line, _ = _lossless_reference(args.lossless_ref, np.asarray(origins, np.int64), dev,
                                                       mv_pack=total_pack.get('lossless_mv_pack'))
                print(ref_line)
            elif hasattr(args, 'lossless_ref'):
                print(f'[Info] the lossless_lod_pack of {args.input} refers to no other cloud; --lossless_ref '
                      f'{args.lossless_ref} is not read')
            words, counts = llp.decode_occupancy(net, latents, total_pack['lossless_lod_pack'], *ref, level=level, batch=batch)
        except ValueError as e:
            raise SystemExit(f"decode --lossless_lod {level}: {e}")
        pts = llp.points_from_words(words, counts, origins, level)
        print('[LosslessLoD] level: %d points: %d' % (level, pts.shape[0]))
    elif lod_side is not None:              # a coarser level of detail: the trunk stops at the level's head
        level, t = lod, lod_side['t'][lod - 1]
        pts, counts = reconstruct_points_lod(net, latents, origins, lod, t, batch=batch)
        print(lp.lod_line(lod, t, pts.shape[0]))
    else:
        thh, block_counts, used = args.thh, None, []
        side = total_pack.get('thh_pack')
        if side is None and args.thh_mode not in (None, 'fixed'):
            raise SystemExit(f"decode --thh_mode {args.thh_mode}: {args.input} carries no thh_pack (it was encoded "
                             f"without --thh_mode); decode it with --thh instead")
        if side is not None and args.thh_mode != 'fixed':
            from nvfpcc_amd import thh_select as ts
            mode, value = ts.read_thh_pack(side)
            if mode == 'block-count':
                block_counts = value[:n]
            else:
                thh = value
                print(ts.threshold_line(mode, t=thh))
        pts, counts = reconstruct_points(net, latents, origins, thh, batch=batch, block_counts=block_counts, thh_out=used)
        if block_counts is not None:
            print(ts.threshold_line('block-count', block_counts=block_counts, thresholds=torch.cat(used).cpu().numpy()))
    ply_io.write_ply(out_fn, pts, fmt=fmt, device=dev)
    if hasattr(args, 'source_frame'):       # the same points in the input's frame; at level L the step is s 2^L
        ply_io.write_ply_float(out_fn.replace('rc_dec', 'rc_dec_src', 1), vx.to_source(pts, lattice, dev, level=level), fmt)
    if args.ref_ply is not None:
        _print_pc_error(args, pts, dev, bits=_pack_bits(total_pack, origins), lod=level, lattice=lattice)


def _decoder_from_pack(args, total_pack, dev, net=None, lod_side=None):
    """The decoder and the latents a pack's bytes hold: the de-quantised kernels and the as-is parameters of
    net_weight_pack (and the coarse heads of a read lod_pack) loaded into `net` (a fresh one when absent), and the
    latents of latent_pack.  -> (net on dev, latents on dev)."""
    from nvfpcc_amd import weight_codec, latent_codec
    if net is None:
        net = _build_net(args, torch.device('cpu'))
    wp = total_pack['net_weight_pack']
    dec_pool = weight_codec.entropy_decode(wp['bit_stream'], wp['inv_codebook'], wp['element_length'], wp['shape_list'])
    nd_ = {}
    for k, v in zip(wp['keys_quantize'], dec_pool):
        nd_[k] = torch.from_numpy(v).float() / args.qp
    for k, v in zip(wp['keys_code_as_is'], wp['as_is_pool']):
        nd_[k] = torch.from_numpy(np.asarray(v)).float()
    if lod_side is not None:
        nd_.update(lod_side['state'])
    net.load_state_dict(nd_, strict=False)
    net = net.to(dev)
    latents = latent_codec.arithmetic_dec(total_pack['latent_pack']).to(dev)
    return net, latents


def lossless_refusals(args, total_pack):
    """decode --lossless: what cannot be served exits here with its reason.  total_pack None: the flags alone."""
    if not getattr(args, 'lossless', False):
        return
    if getattr(args, 'lod', 0):
        raise SystemExit("decode: --lossless and --lod exclude each other: lossless_pack codes the 32^3 occupancy, a "
                         "coarser level of detail is lossy by construction")
    if total_pack is not None and 'lossless_pack' not in total_pack:
        raise SystemExit(f"decode --lossless: {args.input} carries no lossless_pack (it was encoded without --lossless)")


def lossless_ctx_refusals(args):
    """encode --lossless_ctx: it chooses the contexts of --lossless_lod and means nothing without it; the contexts
    `inter` and the cloud of --lossless_ref come together, and not inside a group of frames."""
    if hasattr(args, 'lossless_ctx') and getattr(args, 'lossless_lod', None) is None:
        raise SystemExit(f"encode: --lossless_ctx {args.lossless_ctx} chooses the contexts of --lossless_lod; give "
                         f"--lossless_lod too")
    inter = getattr(args, 'lossless_ctx', None) == 'inter'
    if inter and not hasattr(args, 'lossless_ref'):
        raise SystemExit("encode: --lossless_ctx inter codes the voxels under a reference cloud; name it with "
                         "--lossless_ref (the previous frame's rc_dec.ply, say)")
    if hasattr(args, 'lossless_ref') and not inter:
        raise SystemExit(f"encode: --lossless_ref {args.lossless_ref} is the reference of --lossless_ctx inter; give "
                         f"--lossless_lod --lossless_ctx inter too")
    if inter and hasattr(args, 'gof'):
        raise SystemExit("encode: --gof and --lossless_ctx inter exclude each other: a frame that refers to its "
                         "predecessor inside a group is not coded; encode the frames one by one with --lossless_ref")
    if hasattr(args, 'lossless_mv'):
        if not inter:
            raise SystemExit(f"encode: --lossless_mv {args.lossless_mv} moves the reference of --lossless_ctx inter; give "
                             f"--lossless_lod --lossless_ctx inter --lossless_ref too")
        if not 1 <= args.lossless_mv <= 8:
            raise SystemExit(f"encode: --lossless_mv {args.lossless_mv}: the search radius is 1..8 voxels")


def lossless_lod_refusals(args, total_pack):
    """decode --lossless_lod: what cannot be served exits here with its reason.  total_pack None: the flags alone."""
    level = getattr(args, 'lossless_lod', None)
    if level is None:
        return
    if getattr(args, 'lod', 0):
        raise SystemExit("decode: --lossless_lod and --lod exclude each other: --lossless_lod 1 | 2 is the exact coarse "
                         "cloud, --lod the coarse heads' lossy one")
    if getattr(args, 'lossless', False):
        raise SystemExit("decode: --lossless_lod and --lossless exclude each other: each decodes its own side pack into "
                         "rc_dec.ply")
    if total_pack is not None and 'lossless_lod_pack' not in total_pack:
        raise SystemExit(f"decode --lossless_lod {level}: {args.input} carries no lossless_lod_pack (it was encoded "
                         f"without --lossless_lod)")
    if total_pack is not None and 'lossless_mv_pack' in total_pack and bytes(total_pack['lossless_lod_pack'][:1]) != b'\x04':
        raise SystemExit(f"decode --lossless_lod {level}: {args.input} carries a lossless_mv_pack, the vectors of a "
                         f"reference cloud, but its lossless_lod_pack is not version 4 and refers to none")


def _pack_bits(total_pack, origins):
    """Bits per axis of the cloud a pack holds: octree_pack's header byte (the leaf level D) + 5, or for raw origins
    the smallest of 10 / 11 / 12 whose volume holds every 32^3 leaf cube."""
    if 'octree_pack' in total_pack:
        return int(total_pack['octree_pack'][0]) + 5
    top = int(np.max(origins)) + 31 if len(origins) else 0
    for bits in (10, 11, 12):
        if top < (1 << bits):
            return bits
    raise SystemExit(f"--ref_ply: the pack's leaf cubes reach coordinate {top}, beyond 12 bits per axis")


def _print_pc_error(args, pts, dev, bits=10, lod=0, lattice=None):
    """--ref_ply: symmetric D1 / D2 geometry PSNR of the written cloud against the original (nvfpcc_amd.pc_metrics);
    `bits` is the domain of both clouds, and the peak of the PSNR is 2^bits - 1.  lod > 0: `pts` lie on the lattice of
    bits - lod bits per axis; the original is reduced to it (>> lod, duplicates removed: its normals do not survive,
    D2 uses estimated ones) and bits - lod is the domain and the peak.  lattice (encode --voxelize, decode of a pack with
    vox_pack): the original has float coordinates; it is voxelised under that lattice, never under a fit of its own,
    and scored on the lattice (its normals do not survive the merging of points either)."""
    if args.ref_ply is None:
        return
    from nvfpcc_amd import ply_io
    from nvfpcc_amd.pc_metrics import geometry_psnr
    if lattice is not None:
        from nvfpcc_amd import voxelize as vx
        try:
            ref, ref_normals = vx.voxelize(ply_io.read_ply(args.ref_ply, coords='float')[0], dev, lattice=lattice).points, None
        except (OSError, ValueError) as e:
            raise SystemExit(f"--ref_ply {args.ref_ply}: {e}")
    else:
        ref, ref_normals = ply_io.read_ply(args.ref_ply, device=dev, normals=True)      # ASCII or binary
    if lod:
        from nvfpcc_amd.recon import reduce_to_lattice
        ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else ref
        ref, ref_normals, bits = reduce_to_lattice(ref, lod), None, bits - lod
        print('[PCError] LoD %d: %d reference points on the %d-bit lattice, peak %d' % (lod, ref.shape[0], bits, (1 << bits) - 1))
        # the search index covers 10 to 12 bits per axis; a smaller domain fits the 10-bit one, the peak is the lattice's
        r = geometry_psnr(ref, pts, peak=(1 << bits) - 1, ref_normals=None, device=dev, bits=max(bits, 10))
        print('[PCError] D1 PSNR: %.4f D2 PSNR: %.4f' % (r['d1_psnr'], r['d2_psnr']))
        return
    r = geometry_psnr(ref, pts, ref_normals=ref_normals, device=dev, bits=bits)
    print('[PCError] D1 PSNR: %.4f D2 PSNR: %.4f' % (r['d1_psnr'], r['d2_psnr']))


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("command", choices=["train", "encode", "decode"], help="What to do?")
    p.add_argument("input", nargs="?", help="Input filename.")
    p.add_argument("--checkpoint_dir", default="train", help="Directory where to save/load model checkpoints.")
    p.add_argument("--batchsize", type=int, default=2, help="Batch size for training.")
    p.add_argument("--lambda", type=float, default=0.01, dest="lmbda", help="Lambda for rate-distortion tradeoff.")
    p.add_argument("--load_weights", default="", help="Weights to load")
    p.add_argument("--load_extern", default="", help="Load external weights")
    p.add_argument("--lr", type=float, default=1e-4, help="Learning rate.")
    p.add_argument("--alpha", type=float, default=200, help="Alpha.")
    # type=bool as in the reference: any non-empty string is True (NVFPCC.py:684-692, 710)
    p.add_argument("--use_coords", type=bool, default=False, help="Use coords?")
    p.add_argument("--real", type=bool, default=False, help="Real compression?")
    p.add_argument("--dsep", type=bool, default=False, help="Use depth-separable conv?")
    p.add_argument("--stat_latent", type=bool, default=False, help="(unused)")
    p.add_argument("--stat_net", type=bool, default=False, help="(unused)")
    p.add_argument("--w1", type=float, default=1, dest="w1", help="W1 for rate-distortion tradeoff.")
    p.add_argument("--w2", type=float, default=1, dest="w2", help="W2 for rate-distortion tradeoff.")
    p.add_argument("--notes", type=str, default="Hello", dest="notes", help="Leave a note?")
    p.add_argument("--load_meta", type=str, default="", dest="load_meta", help="Load a meta init")
    p.add_argument('--shuffle', type=bool, default=False, dest="shuffle", help="Shuffle the dataset randomly?")
    p.add_argument("--phase_change", type=int, default=100, dest="phase_change", help="Phase change epoch.")
    p.add_argument("--wemb", type=float, default=5, dest="wemb", help="Weight for emb lr.")
    p.add_argument('--ch', type=int, default=8, dest="ch", help="# channels in latent")
    p.add_argument("--load_emb", type=str, default="", dest="load_emb", help="Load an emb")
    p.add_argument("--chanstr", type=str, default="8,16,8,8", dest="chanstr", help="Control channels in the compnet")
    p.add_argument("--thh", type=float, default=0.6, dest="thh", help="Threshold.")
    p.add_argument('--pack_fn', default='pack.pk', help='package filename.')
    p.add_argument('--N', default=917, help='Number of leaves nodes.')
    p.add_argument('--qp', type=float, default=16, help='Quantization parameter used for net weights.')
    # additions
    p.add_argument('--device', default='cuda', help='HIP device (the reference hard-codes cuda).')
    p.add_argument('--epochs', type=int, default=501, help='Number of epochs (the reference hard-codes 501).')
    p.add_argument('--seed', type=int, default=0, help='Seed of the counter RNG behind the q=1 / latent noise.')
    p.add_argument('--thh_mode', default=None, choices=['fixed', 'count', 'block-count', 'd1'],
                   help='How the occupancy threshold is chosen.  Absent: --thh, nothing added to the pack.  encode: '
                        'count = keep as many voxels as the input has points; block-count = the same per block; '
                        'd1 = the candidate with the best symmetric D1 PSNR.  The choice travels in the pack '
                        '(thh_pack) and decode uses it; decode --thh_mode fixed ignores it and uses --thh.')
    # opt-in switches: absent from the namespace unless given, so a command line without them parses as it always did
    p.add_argument('--from_ply', action='store_true', default=argparse.SUPPRESS,
                   help='train / encode: the input is the cloud itself (ASCII or binary PLY, 10-bit coordinates); it is '
                        'pre-processed on the device and no *_l5_*.npy file is read or written.')
    p.add_argument('--bits', type=int, choices=[10, 11, 12], default=argparse.SUPPRESS,
                   help='train / encode with --from_ply: bits per axis of the cloud (10 when absent).  The leaf cubes '
                        'stay 32^3, so 11 and 12 make the octree one and two levels deeper; decode needs no flag.')
    p.add_argument('--pack_octree', action='store_true', default=argparse.SUPPRESS,
                   help='encode: carry the leaf cubes in the pack as octree occupancy bytes (octree_pack, counted in '
                        'Gross bpp) instead of raw origins; decode then needs no --N.')
    p.add_argument('--pack_lod', action='store_true', default=argparse.SUPPRESS,
                   help='encode: carry the two coarse classifier heads and their thresholds in the pack (lod_pack, '
                        'counted in Gross bpp), so that decode --lod can stop at a coarser level of detail; also writes '
                        'rc_enc_lod1.ply / rc_enc_lod2.ply.')
    p.add_argument('--lod_heads', default=argparse.SUPPRESS,
                   help='encode --pack_lod: checkpoint that holds the coarse heads conv1_cls / conv0_cls (the one '
                        'training wrote; manipulate_weights.py drops them).  Absent: --load_weights must hold them.')
    p.add_argument('--lod', type=int, choices=[1, 2], default=argparse.SUPPRESS,
                   help='decode: level of detail.  1 = 16^3 per block (half resolution), 2 = 8^3 (quarter); the trunk '
                        'stops at that level and rc_dec.ply lies on the lattice of bits - lod bits per axis.  Needs a '
                        'pack encoded with --pack_lod.')
    p.add_argument('--lossless', action='store_true', default=argparse.SUPPRESS,
                   help='encode: also code the true occupancy of every leaf block under the decoder\'s probabilities '
                        '(lossless_pack, counted in Gross bpp).  decode: write exactly the input\'s voxels to rc_dec.ply '
                        'from a pack encoded with it; excludes --lod.')
    p.add_argument('--lossless_lod', type=int, nargs='?', choices=[0, 1, 2], const=0, default=argparse.SUPPRESS,
                   help='encode (no value): also code the true occupancy coarse to fine (lossless_lod_pack, counted in '
                        'Gross bpp).  decode --lossless_lod L: write exactly the input\'s voxels (0) or exactly their '
                        'reduction to bits - L bits per axis (1, 2) to rc_dec.ply, from a prefix of the same stream; '
                        'excludes --lod and --lossless.')
    p.add_argument('--lossless_ctx', choices=['field', 'nbr', 'inter'], default=argparse.SUPPRESS,
                   help='encode --lossless_lod: the contexts of the voxels.  field (the default): the decoder\'s field '
                        'alone.  nbr: also the exact 16^3 occupancy of the parent cell\'s neighbours, which the decoder '
                        'holds before the first voxel (fewer bits; decode tells the two apart by the pack).  inter: '
                        'also the cloud of --lossless_ref, which both sides hold (far fewer bits where the scene stands '
                        'still; decode needs the same cloud).')
    p.add_argument('--lossless_ref', default=argparse.SUPPRESS,
                   help='encode --lossless_lod --lossless_ctx inter / decode --lossless_lod of such a pack: the reference '
                        'cloud (ASCII or binary PLY), normally the previous frame\'s rc_dec.ply.  The pack carries a '
                        'digest of it on this frame\'s blocks: decode refuses any other cloud.')
    p.add_argument('--lossless_mv', type=int, metavar='R', default=argparse.SUPPRESS,
                   help='encode --lossless_lod --lossless_ctx inter: block motion compensation.  Each block is coded under '
                        'the reference cloud moved by its own integer vector, found by an exhaustive search of radius R '
                        '(1..8 voxels); the vectors travel in lossless_mv_pack (counted in Gross bpp).  decode needs no '
                        'flag.')
    p.add_argument('--gof', type=int, default=argparse.SUPPRESS,
                   help='train / encode: a group of F frames under one decoder.  `input` is then the pattern of their '
                        'names with one %%d or %%0<n>d (seq_%%04d.ply); the frames are numbered from --frame_start.  encode '
                        'writes one pack (the weights once, a frame pack each) and rc_enc_<number>.ply per frame.')
    p.add_argument('--frame_start', type=int, default=argparse.SUPPRESS,
                   help='train / encode --gof: number of the first frame (0 when absent).')
    p.add_argument('--frame', type=int, default=argparse.SUPPRESS,
                   help='decode of a group: the frame of that number alone, into rc_dec.ply; nothing of another frame is '
                        'read.  Absent: every frame, into rc_dec_<number>.ply (--ref_ply is then a pattern too).')
    p.add_argument('--freeze_decoder', action='store_true', default=argparse.SUPPRESS,
                   help='train: fit the latents of the input under the decoder of --load_weights (a quantised checkpoint), '
                        'which does not move; --epochs latent steps, every block keeps the best rounded latents seen.  '
                        'Writes <checkpoint_dir>/<epochs - 1>_emb.ckpt.')
    p.add_argument('--ref_pack', default=argparse.SUPPRESS,
                   help='A pack that carries the decoder.  encode: write a latents-only pack (ref_pack, 33 bytes, in place '
                        'of net_weight_pack) after checking that --load_weights is that decoder.  decode: the reference '
                        'of a latents-only pack.  train --freeze_decoder with --load_emb: warm-start every block from '
                        'the reference\'s row of the same or the nearest origin.')
    p.add_argument('--ply_format', choices=['ascii', 'binary'], default=argparse.SUPPRESS,
                   help='encode / decode: format of the rc_*.ply files written.  ascii (also when absent): double x y z '
                        'as text; binary: binary_little_endian with float x y z.')
    p.add_argument('--voxelize', action='store_true', default=argparse.SUPPRESS,
                   help='train / encode --from_ply: the input has float coordinates in a frame of its own and may repeat '
                        'points.  It is voxelised on the device (nvfpcc_amd.voxelize) to --bits bits per axis, under the '
                        'lattice of --vox_step / --vox_origin or under its own fit; every count downstream is the number '
                        'of distinct voxels.  encode carries the lattice in the pack (vox_pack, 34 bytes, counted in '
                        'Gross bpp).  Give train and encode the same flags.')
    from nvfpcc_amd.voxelize import add_lattice_arguments
    add_lattice_arguments(p)
    p.add_argument('--source_frame', action='store_true', default=argparse.SUPPRESS,
                   help='decode of a pack with vox_pack: also write rc_dec_src.ply (rc_dec_src_<number>.ply for a group), '
                        'the decoded points in the input\'s frame, origin + q * step, as float64 in --ply_format.  With '
                        '--lod / --lossless_lod L the step is 2^L times the pack\'s.')
    p.add_argument('--ref_ply', default=None,
                   help='Original cloud (ASCII or binary PLY): encode / decode also print its D1 / D2 geometry PSNR.')
    return p


if __name__ == "__main__":
    _banner()
    args = build_parser().parse_args()
    {"train": train, "encode": encode, "decode": decode}[args.command](args)
