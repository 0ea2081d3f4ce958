"""CPU-side checks of the C-ABI boundary: the library builds, loads, and exports every symbol
include/nvf_hip.h declares (no compute calls -- there is no GPU in the build container)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:            # (this file is also the child process of trunk_refusals below)
    sys.path.insert(0, ROOT)

from nvfpcc_amd import _lib
from nvfpcc_amd.build import build


def declared_symbols(header="nvf_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nvf_[a-zA-Z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    path = build()
    assert os.path.isfile(path)
    h = ctypes.CDLL(path)
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(h, n), f"{n} declared in include/nvf_hip.h but not exported"


def test_python_prototypes_cover_the_header():
    assert sorted(_lib.PROTOTYPES) == declared_symbols()
    assert _lib.lib().nvf_version() >= 100


def test_workspace_queries_need_no_gpu():
    h = _lib.lib()
    assert h.nvf_wgrad_workspace(16, 8, 8, 4, 32, 32, 32) >= 8 * 8 * 64 * 4
    assert h.nvf_channel_sum_workspace(8) > 0
    assert h.nvf_gdn_bwd_workspace(8) > 0
    assert h.nvf_reduce_workspace() > 0


def test_request_struct_layout_matches_the_library():
    """A mismatch between the ctypes Structure and the header would otherwise first show as a fault on a GPU."""
    assert ctypes.sizeof(_lib.NvfTrunkWgrads) == _lib.lib().nvf_trunk_wgrads_bytes() == 152
    assert ctypes.sizeof(_lib.NvfLayerDesc) == _lib.lib().nvf_layer_desc_size() == 88
    import numpy as np
    assert np.dtype(_lib.NvfLayerDesc).itemsize == 88      # the layer table's row (engine._DESC)


# ---- refusals of nvf_wgrad_trunk_partial: every one returns before any HIP call, so dummy addresses will do ----------
EINVAL, EWORKSPACE = -1, -2
DUMMY = 0x1000          # a non-null address nobody dereferences: array entries are only compared with NULL on the host
HEADS = ("head_dls", "head_xs", "head_slabs", "head_nslabs", "head_max_slabs")
SUMS = ("sum_xs", "sum_outs", "sum_channels", "sum_spatials", "sum_n", "sum_workspace", "sum_workspace_bytes")
SUM_BYTES = 128 * 24 * 4   # nvf_multi_channel_sum_workspace(8 + 16 channels)


def _arrays():
    """Host arrays behind a complete request (five jobs, bias, heads, sums, coefficients); kept alive by the caller."""
    ptrs = lambda n: (ctypes.c_void_p * n)(*[DUMMY] * n)
    return dict(ps=ptrs(5), qs=ptrs(5), slabs=ptrs(5), nslabs=(ctypes.c_int * 5)(), bias_slabs=ptrs(3),
                head_dls=ptrs(3), head_xs=ptrs(3), head_slabs=ptrs(3), head_nslabs=(ctypes.c_int * 3)(),
                sum_xs=ptrs(2), sum_outs=ptrs(2), sum_channels=(ctypes.c_int * 2)(8, 16),
                sum_spatials=(ctypes.c_int * 2)(64, 512))


def _request(arrs, drop=(), **fields):
    """A complete request over ``arrs`` minus the fields named in ``drop``, with ``fields`` set on top."""
    vals = {k: ctypes.addressof(v) for k, v in arrs.items()}
    vals.update(batch=4, njobs=5, head_max_slabs=512, sum_n=2, sum_workspace=DUMMY, sum_workspace_bytes=SUM_BYTES,
                coef_src=DUMMY, coef_live=DUMMY)
    vals.update(fields)
    return _lib.NvfTrunkWgrads(**{k: v for k, v in vals.items() if k not in drop})


def _null_entry(name, j):
    def edit(arrs):
        arrs[name][j] = None
    return edit


# name -> (expected code, fields dropped from the complete request, fields set, edit of the arrays)
TRUNK_REFUSALS = {
    **{"null " + f: (EINVAL, (f,), {}, None) for f in ("ps", "qs", "slabs", "nslabs")},
    **{"null %s[%d]" % (f, j): (EINVAL, (), {}, _null_entry(f, j)) for f, j in
       (("ps", 0), ("qs", 2), ("slabs", 4), ("head_dls", 1), ("head_xs", 2), ("head_slabs", 0), ("sum_xs", 1),
        ("sum_outs", 0))},
    "batch 0": (EINVAL, (), {"batch": 0}, None),
    "batch -1": (EINVAL, (), {"batch": -1}, None),
    **{"njobs %d" % n: (EINVAL, (), {"njobs": n}, None) for n in (0, 2, 4, 6)},
    "heads with three jobs": (EINVAL, SUMS + ("bias_slabs", "coef_src", "coef_live"), {"njobs": 3}, None),
    "bias with three jobs": (EINVAL, HEADS + SUMS + ("coef_src", "coef_live"), {"njobs": 3}, None),
    "sums without heads": (EINVAL, HEADS + ("coef_src", "coef_live"), {}, None),
    "coefficients without sums": (EINVAL, SUMS, {}, None),
    "coef_src alone": (EINVAL, ("coef_live",), {}, None),
    "coef_live alone": (EINVAL, ("coef_src",), {}, None),
    **{"heads without " + f: (EINVAL, (f,), {}, None) for f in HEADS},
    "head_max_slabs -1": (EINVAL, (), {"head_max_slabs": -1}, None),
    **{"sums without " + f: (EINVAL, (f,), {}, None) for f in SUMS[:-1]},
    "sums without sum_workspace_bytes": (EWORKSPACE, ("sum_workspace_bytes",), {}, None),
    "sum workspace one byte short": (EWORKSPACE, (), {"sum_workspace_bytes": SUM_BYTES - 1}, None),
    "13 sum tensors": (EINVAL, (), {"sum_n": 13}, None),
    "a sum tensor without channels": (EINVAL, (), {}, lambda arrs: arrs["sum_channels"].__setitem__(1, 0)),
}


def _new_ctx(h):
    buf = ctypes.create_string_buffer(h.nvf_step_ctx_bytes())
    assert h.nvf_step_ctx_init(buf) == 0
    return buf


def _queue_tail(h, ctx, batch, c, spatial):
    """A latent tail of dummy addresses in ``ctx`` (host code only)."""
    d = DUMMY
    return h.nvf_latent_tail_queue(ctx, d, None, d, d, None, d, d, d, None, 1.0, 0, 0, 0, None, d, d, d, d, d, d, d, d, d,
                                   batch, c, spatial)


def _queue_stem(h, ctx, batch, ch):
    """A stem backward of dummy addresses in ``ctx``, whose finals queue gets opened (host code only)."""
    d = DUMMY
    out, n = ctypes.c_void_p(), ctypes.c_int()
    assert h.nvf_finals_begin(ctx) == 0
    return h.nvf_stem_bwd_queue(ctx, d, d, d, d, d, d, d, d, d, d, d, ctypes.byref(out), ctypes.byref(n), ctypes.byref(out),
                                d, h.nvf_stem_bwd_workspace_for(batch, ch, 8, 16), d, batch, ch, 8, 16, None)


def _trunk_refusal_codes():
    """Return code of every case, what is still queued in a context after a refusal, and the reductions' refusals.
    Run in a child process that sees no GPU (trunk_refusals): a call that was wrongly accepted then fails in the runtime
    instead of launching a kernel on dummy addresses."""
    h = _lib.lib()
    out = {"null request": h.nvf_wgrad_trunk_partial(None, None, None)}
    for name, (_, drop, fields, edit) in TRUNK_REFUSALS.items():
        arrs = _arrays()
        if edit:
            edit(arrs)
        out[name] = h.nvf_wgrad_trunk_partial(ctypes.byref(_request(arrs, drop, **fields)), None, None)
    # a refusal leaves a queued tail queued ...
    arrs, ctx = _arrays(), _new_ctx(h)
    assert _queue_tail(h, ctx, 4, 8, 8) == 0
    out["tail: refused"] = h.nvf_wgrad_trunk_partial(ctypes.byref(_request(arrs, batch=0)), ctx, None)
    out["tail: still pending"] = h.nvf_latent_tail_pending(ctx)
    # ... and the stem / tail consistency check comes before either flag is cleared: a stem backward without a tail,
    # with three jobs, with another batch, with a tail of another size
    for name, tail, fields in (("no tail", None, {}), ("three jobs", (4, 8, 8), {"njobs": 3}), ("batch", (4, 8, 8), {"batch": 5}),
                               ("tail size", (4, 8, 4), {})):
        ctx = _new_ctx(h)
        assert _queue_stem(h, ctx, 4, 8) == 0 and (tail is None or _queue_tail(h, ctx, *tail) == 0)
        drop = HEADS + SUMS + ("bias_slabs", "coef_src", "coef_live") if fields.get("njobs") == 3 else ()
        out["stem, %s: refused" % name] = h.nvf_wgrad_trunk_partial(ctypes.byref(_request(arrs, drop, **fields)), ctx, None)
        out["stem, %s: still pending" % name] = [h.nvf_stem_bwd_pending(ctx), h.nvf_latent_tail_pending(ctx)]
    # the four slab reductions
    ptrs, ints = (ctypes.c_void_p * 17)(*[DUMMY] * 17), (ctypes.c_int * 17)(*[1] * 17)
    ctx, blank = _new_ctx(h), ctypes.create_string_buffer(h.nvf_step_ctx_bytes())
    adam = _lib.NvfAdamFuse(g_base=DUMMY, p_base=DUMMY, m_base=DUMMY, v_base=DUMMY, n=64, beta1=0.9, beta2=0.999, eps=1e-8)
    tail = _lib.NvfStepTail(p=DUMMY, g=DUMMY, m=DUMMY, v=DUMMY, n=64)
    jobs = lambda n: (ptrs, ptrs, ints, ints, n)
    finals_tail = lambda n, c: h.nvf_wgrad_reduce_finals_tail(*jobs(n), None, ctypes.byref(adam), c, ctypes.byref(tail), None,
                                                              0, None)
    for n in (0, 17):
        out["reduce_multi: n = %d" % n] = h.nvf_wgrad_reduce_multi(*jobs(n), None)
        out["reduce_finals: n = %d" % n] = h.nvf_wgrad_reduce_finals(*jobs(n), None, ctx, None)
        out["reduce_finals_tail: n = %d" % n] = finals_tail(n, ctx)
        out["reduce_multi_and_sums_fused: n = %d" % n] = h.nvf_wgrad_reduce_multi_and_sums_fused(
            *jobs(n), None, None, ptrs, ptrs, ints, ints, 2, 4, DUMMY, 1 << 20, None, None)
    for what, c in (("no", None), ("a blank", blank)):
        out["reduce_finals: %s context" % what] = h.nvf_wgrad_reduce_finals(*jobs(3), None, c, None)
        out["reduce_finals_tail: %s context" % what] = finals_tail(3, c)
    out["reduce_multi: nothing to add"] = h.nvf_wgrad_reduce_multi(ptrs, ptrs, (ctypes.c_int * 17)(), ints, 16, None)
    # the split optimiser's two launches as one call: whatever its SECOND launch would refuse, refused before the first
    no_n = _lib.NvfStepTail(p=DUMMY, g=DUMMY, m=DUMMY, v=DUMMY, n=0)
    past = (ctypes.c_int64 * 2)(0, 65)
    split = lambda n, a, c, t, rg, nrg: h.nvf_wgrad_reduce_sums_fused_flush_tail(
        *jobs(n), None, a, ptrs, ptrs, ints, ints, 2, 4, DUMMY, 1 << 20, c, t, rg, nrg, None)
    for name, args in (("no optimiser", (3, None, ctx, ctypes.byref(tail), None, 0)),
                       ("no tail", (3, ctypes.byref(adam), ctx, None, None, 0)),
                       ("a blank context", (3, ctypes.byref(adam), blank, ctypes.byref(tail), None, 0)),
                       ("a tail of no parameters", (3, ctypes.byref(adam), ctx, ctypes.byref(no_n), None, 0)),
                       ("a range past the parameters", (3, ctypes.byref(adam), ctx, ctypes.byref(tail), past, 1)),
                       ("17 ranges", (3, ctypes.byref(adam), ctx, ctypes.byref(tail), past, 17)),
                       ("17 jobs", (17, ctypes.byref(adam), ctx, ctypes.byref(tail), None, 0))):
        out["split optimiser: " + name] = split(*args)
    return out


@pytest.fixture(scope="module")
def trunk_refusals():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, text=True, check=True)
    return json.loads(r.stdout.splitlines()[-1])


@pytest.mark.parametrize("case", ["null request"] + list(TRUNK_REFUSALS))
def test_trunk_launch_refuses(trunk_refusals, case):
    assert trunk_refusals[case] == (TRUNK_REFUSALS[case][0] if case in TRUNK_REFUSALS else EINVAL)


def test_a_refused_trunk_launch_leaves_the_context_as_it_was(trunk_refusals):
    assert trunk_refusals["tail: refused"] == EINVAL and trunk_refusals["tail: still pending"] == 1
    for name, tail in (("no tail", 0), ("three jobs", 1), ("batch", 1), ("tail size", 1)):
        assert trunk_refusals["stem, %s: refused" % name] == EINVAL, name
        assert trunk_refusals["stem, %s: still pending" % name] == [1, tail], name


def test_reduction_entry_points_refuse_bad_job_counts_and_contexts(trunk_refusals):
    """n = 0 and n = 17 for each of the four; an uninitialised context for the two that take the queue out of one; and
    nvf_wgrad_reduce_multi has nothing to launch, and says NVF_OK, when every job was written directly."""
    codes = {k: v for k, v in trunk_refusals.items() if k.startswith("reduce")}
    assert len(codes) == 2 * 4 + 2 * 2 + 1
    assert codes.pop("reduce_multi: nothing to add") == 0
    assert set(codes.values()) == {EINVAL}, codes


def test_the_split_optimisers_one_call_refuses_before_its_first_launch(trunk_refusals):
    """nvf_wgrad_reduce_sums_fused_flush_tail = the slab reduction with fused Adam + nvf_finals_flush_tail: a request whose
    second launch would be refused must not run the first (half of the parameters updated).  Seven such requests; the
    child process sees no GPU, so one wrongly accepted fails in the runtime instead of returning NVF_EINVAL."""
    codes = {k: v for k, v in trunk_refusals.items() if k.startswith("split optimiser")}
    assert len(codes) == 7 and set(codes.values()) == {EINVAL}, codes


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from nvfpcc_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.maxpool2(torch.zeros(1, 1, 4, 4, 4))


def test_codec_library_exports_its_header():
    from nvfpcc_amd.build import build_codec
    h = ctypes.CDLL(build_codec())
    names = declared_symbols("nvf_codec.h")
    assert names == ["nvf_ac_decode", "nvf_ac_encode", "nvf_codec_version"]
    for n in names:
        assert hasattr(h, n)


if __name__ == "__main__":
    print(json.dumps(_trunk_refusal_codes()))
