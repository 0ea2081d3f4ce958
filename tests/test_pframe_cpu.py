"""nvfpcc_amd.pframe without a device: the latents-only pack's framing (split / join / digest) and the warm start."""
import copy
import pickle

import numpy as np
import pytest
import torch

from nvfpcc_amd import gof, pframe
from tests.test_gpu_lod_cli import same


def weight_pack(seed=0):
    """A net_weight_pack of the shape weight_codec.enc_dec_from_file writes, small."""
    r = np.random.default_rng(seed)
    return {'bit_stream': bytes(r.integers(0, 256, 40, dtype=np.uint8)), 'inv_codebook': {'0': 0, '10': -1, '110': 1, '111': 2},
            'element_length': 24, 'shape_list': [(2, 3, 1, 1, 1), (3, 2, 1, 1, 3)],
            'as_is_pool': [r.standard_normal((1, 3, 1, 1, 1)).astype(np.float32), r.standard_normal(3).astype(np.float32),
                           np.float32(2.0 ** -36)],
            'keys_quantize': ['reconstructor.up0.kernel', 'reconstructor.conv0.kernel'],
            'keys_code_as_is': ['entropy_coder.sigma', 'entropy_coder.mu', 'reconstructor.activation.pedestal']}


def frame_pack(seed, n=4):
    r = np.random.default_rng(100 + seed)
    return {'origins': (32 * r.integers(0, 8, (n, 3))).astype(np.int16),
            'latent_pack': {'latent_byte_stream': bytes(r.integers(0, 256, 9, dtype=np.uint8)), 'shape': (n, 3, 2, 2, 2),
                            'sigma': torch.ones(1, 3, 1, 1, 1), 'mu': torch.zeros(1, 3, 1, 1, 1)},
            'lossless_pack': bytes(r.integers(0, 256, 17, dtype=np.uint8))}


def plain_pack():
    return {'net_weight_pack': weight_pack(), **frame_pack(0)}


def group_pack():
    frames = [frame_pack(k) for k in range(3)]
    return {'net_weight_pack': weight_pack(), 'gof_pack': gof.write_gof_pack(5, [4, 4, 4], [100, 110, 120]), 'frames': frames}


@pytest.mark.parametrize("make", [plain_pack, group_pack])
def test_split_join_round_trip(make):
    pack = make()
    p = pframe.split(pack)
    assert list(p) == ['ref_pack'] + [k for k in pack if k != 'net_weight_pack']
    assert p['ref_pack'] == b'\x01' + pframe.digest(pack['net_weight_pack']) and len(p['ref_pack']) == pframe.REF_PACK_BYTES == 33
    assert pframe.is_p_pack(p) and not pframe.is_p_pack(pack)
    # the reference is ANOTHER pack that carries the same decoder (here: another frame's plain pack), pickled in between
    ref = pickle.loads(pickle.dumps({'net_weight_pack': weight_pack(), **frame_pack(9)}))
    joined = pframe.join(pickle.loads(pickle.dumps(p)), ref)
    assert same(joined, pack) and list(joined)[0] == 'net_weight_pack'
    if 'gof_pack' in pack:
        assert same(gof.extract(joined, 1), gof.extract(pack, 1))
        assert gof.account(p)['weight_bits'] == 8 * 33 and gof.account(pack)['weight_bits'] == 8 * 40
        assert gof.account(p)['gross_bpp'] == (8 * 33 + gof.account(pack)['latent_bits'] + gof.account(pack)['side_bits']
                                               + gof.account(pack)['gof_bits']) / 330.0


def test_digest_is_stable_and_sees_every_field():
    wp = weight_pack()
    d = pframe.digest(wp)
    assert isinstance(d, bytes) and len(d) == 32
    assert pframe.digest(pickle.loads(pickle.dumps(wp))) == d and pframe.digest(weight_pack()) == d
    assert pframe.digest(dict(reversed(list(wp.items())))) == d, "key order of the dict is not part of the decoder"
    seen = {d}

    def changed(**kw):
        other = pframe.digest({**copy.deepcopy(wp), **kw})
        assert other not in seen, kw
        seen.add(other)
    stream = bytearray(wp['bit_stream'])
    stream[7] ^= 1
    changed(bit_stream=bytes(stream))                                   # one weight byte
    pool = copy.deepcopy(wp['as_is_pool'])
    pool[1][2] = np.nextafter(pool[1][2], np.float32(9))
    changed(as_is_pool=pool)                                            # one as-is value, by one ulp
    changed(as_is_pool=[a.astype(np.float64) if a.ndim else a for a in wp['as_is_pool']])
    changed(inv_codebook={'0': 0, '10': -1, '110': 2, '111': 1})
    changed(element_length=23)
    changed(shape_list=[(3, 2, 1, 1, 1), (3, 2, 1, 1, 3)])
    changed(keys_quantize=['reconstructor.conv0.kernel', 'reconstructor.up0.kernel'])
    changed(keys_code_as_is=['entropy_coder.mu', 'entropy_coder.sigma', 'reconstructor.activation.pedestal'])


def test_every_refusal_raises_value_error():
    pack = plain_pack()
    p = pframe.split(pack)
    other = {'net_weight_pack': weight_pack(1), **frame_pack(3)}
    with pytest.raises(ValueError, match="not the one"):
        pframe.join(p, other)                                           # digest mismatch
    with pytest.raises(ValueError, match="do not chain"):
        pframe.join(p, pframe.split(pack))                              # a P pack as reference
    with pytest.raises(ValueError, match="no net_weight_pack"):
        pframe.join(p, frame_pack(0))
    with pytest.raises(ValueError, match="version 2"):
        pframe.join(dict(p, ref_pack=b'\x02' + p['ref_pack'][1:]), pack)
    with pytest.raises(ValueError, match="bytes"):
        pframe.join(dict(p, ref_pack=p['ref_pack'][:-1]), pack)
    with pytest.raises(ValueError, match="no ref_pack"):
        pframe.join(pack, pack)
    with pytest.raises(ValueError, match="no net_weight_pack"):
        pframe.split(p)


def test_warm_start():
    ref_o = np.array([[0, 0, 0], [32, 0, 0], [0, 64, 0], [96, 96, 96], [32, 0, 0]])
    ref_e = torch.arange(5 * 3 * 8, dtype=torch.float32).view(5, 3, 2, 2, 2)
    o = np.array([[0, 64, 0],        # exact: row 2
                  [32, 0, 0],        # exact, twice among the reference's: the lowest index, row 1
                  [96, 96, 64],      # nearest: row 3 (L1 32)
                  [16, 0, 0],        # 16 from rows 0 and 1 (and 4): tie to the lowest index, row 0
                  [32, 32, 0],       # L1 32 from rows 1 and 4 (+y), 32 from row 2 (-y, +x = 64: no) -> row 1
                  [0, 0, 0]])
    got = pframe.warm_start(ref_e, ref_o, o)
    assert isinstance(got, torch.Tensor) and got.dtype == ref_e.dtype and tuple(got.shape) == (6, 3, 2, 2, 2)
    assert torch.equal(got, ref_e[[2, 1, 3, 0, 1, 0]])
    got[0] += 1
    assert ref_e[2, 0, 0, 0, 0] == 48, "a copy, not a view"
    # numpy in, numpy out
    got_np = pframe.warm_start(ref_e.numpy(), ref_o.astype(np.int16), np.array([[40, 40, 40]], np.int16))
    assert isinstance(got_np, np.ndarray) and np.array_equal(got_np[0], ref_e[1].numpy())       # 88 from row 1, 120 from 0, 168 from 3
    assert pframe.warm_start(ref_e, ref_o, np.zeros((0, 3))).shape[0] == 0
    with pytest.raises(ValueError, match="reference"):
        pframe.warm_start(ref_e[:0], np.zeros((0, 3)), o)               # an empty reference
    with pytest.raises(ValueError, match="reference"):
        pframe.warm_start(ref_e[:4], ref_o, o)


def test_pack_origins_of_plain_and_group_packs():
    from nvfpcc_amd import preprocess as pp
    pack, group = plain_pack(), group_pack()
    assert np.array_equal(pframe.pack_origins(pack), pack['origins'].astype(np.int64))
    assert np.array_equal(pframe.pack_origins(group), np.concatenate([f['origins'] for f in group['frames']]).astype(np.int64))
    o = np.array([[0, 0, 0], [32, 0, 0], [992, 992, 960]], np.int16)
    oct_pack = {'net_weight_pack': weight_pack(), 'octree_pack': pp.octree_pack_from_origins(o), 'latent_pack': {}}
    assert sorted(map(tuple, pframe.pack_origins(oct_pack))) == sorted(map(tuple, o.astype(np.int64)))
