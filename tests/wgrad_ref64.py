"""Plain float64 references for the batch-edge tests (tests/test_gpu_batch_edges.py): torch only, no kernel of this
project.

    dw[a, b, k] = sum_{n, i} p[n, a, i] * q[n, b, stride * i - pad + k]

as one float64 einsum per tap k over shifted (strided) slices of the zero-padded q -- the shifted-slice sum of
test_three_head_launches_equal_the_single_head_kernels, for any of the decoder's layers.  It runs where its inputs live
(float64 matmuls of torch on the device for the large batches, on the CPU for the check against torch's autograd in
tests/test_modules_cpu.py) and walks the batch in chunks so that the float64 copies stay small.
"""
import torch
import torch.nn.functional as F


def wgrad_ref64(p, q, k, stride, pad, ends=None, chunk_bytes=128 << 20):
    """float64 dw [A, Bc, k, k, k] of the first ``e`` blocks for every e in ``ends`` (ascending; default: all blocks),
    from ONE pass over the batch: a prefix is the running sum at its end."""
    B, A = p.shape[0], p.shape[1]
    Bc = q.shape[1]
    P = p.shape[2]
    ends = [B] if ends is None else list(ends)
    assert ends == sorted(ends) and 0 < ends[0] and ends[-1] <= B
    span = stride * (P - 1) + 1                     # extent of the positions one tap meets in the padded q
    assert k - 1 + span <= q.shape[2] + 2 * pad
    per_block = 8 * max(A, Bc) * max(P, q.shape[2] + 2 * pad) ** 3
    step = max(1, chunk_bytes // per_block)
    acc = torch.zeros(A, Bc, k, k, k, dtype=torch.float64, device=p.device)
    out, lo = [], 0
    for e in ends:
        while lo < e:
            hi = min(lo + step, e)
            p64 = p[lo:hi].double().reshape(hi - lo, A, -1)
            q64 = F.pad(q[lo:hi].double(), (pad,) * 6)
            for kz in range(k):
                for ky in range(k):
                    for kx in range(k):
                        qs = q64[:, :, kz:kz + span:stride, ky:ky + span:stride, kx:kx + span:stride]
                        acc[:, :, kz, ky, kx] += torch.einsum("nai,nbi->nab", p64, qs.reshape(hi - lo, Bc, -1)).sum(0)
            lo = hi
        out.append(acc.clone())
    return out


def channel_sum_ref64(x, ends=None):
    """float64 sums over batch and space per channel of the first ``e`` blocks for every e in ``ends``."""
    ends = [x.shape[0]] if ends is None else list(ends)
    B, C = x.shape[0], x.shape[1]
    per_block = torch.cat([x[i:i + 64].double().reshape(-1, C, x[0, 0].numel()).sum(2) for i in range(0, B, 64)])  # [B, C]
    return [per_block[:e].sum(0) for e in ends]
