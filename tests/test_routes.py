"""nvfpcc_amd.routes decides which kernel form a layer runs on and which packed weights it holds for that.  It takes no
tensors, so the tables below can be read against the README / DESIGN numbers, and every combination of its inputs can be
checked here, without a device."""
import itertools

from nvfpcc_amd import routes

CLASSES = ("narrow", "wide", "generic")
# (cin, cout, k, pad) of every layer the engine routes, per decoder class (generic: --ch 4 --chanstr 4,8,4,4)
SHAPES = {
    "narrow": dict(latent=(3, 3, 1, 0), up0=(3, 8, 5, 2), conv0=(8, 16, 5, 2), up1=(16, 8, 5, 0), conv1=(8, 8, 4, 0),
                   up2=(8, 8, 5, 0), conv2=(8, 8, 4, 0), conv2_cls=(8, 1, 3, 1), conv1_cls=(8, 1, 3, 1),
                   conv0_cls=(16, 1, 3, 1)),
    "wide": dict(latent=(8, 8, 1, 0), up0=(8, 16, 5, 2), conv0=(16, 32, 5, 2), up1=(32, 16, 5, 0), conv1=(16, 16, 4, 0),
                 up2=(16, 16, 5, 0), conv2=(16, 16, 4, 0), conv2_cls=(16, 1, 3, 1), conv1_cls=(16, 1, 3, 1),
                 conv0_cls=(32, 1, 3, 1)),
    "generic": dict(latent=(4, 4, 1, 0), up0=(4, 4, 5, 2), conv0=(4, 8, 5, 2), up1=(8, 4, 5, 0), conv1=(4, 4, 4, 0),
                    up2=(4, 4, 5, 0), conv2=(4, 4, 4, 0), conv2_cls=(4, 1, 3, 1), conv1_cls=(4, 1, 3, 1),
                    conv0_cls=(8, 1, 3, 1)),
}
TRUNK = ("up0", "conv0", "up1", "conv1", "up2", "conv2")
BATCHES = (1, 16, 32, 33, 64, 65, 512, 917)


def show(r):
    """'form [vN] [ppcN] [+slabs]' of a route: v = the tile variant the C entry point gets (none: the module default)."""
    return (r.form + (" v%d" % r.variant if r.variant is not None else "") + (" ppc%d" % r.ppc if r.ppc else "")
            + (" +slabs" if r.bias_slabs else ""))


def fwd(cls, winograd, name, batch, train, relu=True):
    cin, _, k, _ = SHAPES[cls][name]
    if k == 5:
        return routes.convT_fwd(cls, winograd, name, cin, train)
    return routes.conv_fwd(cls, winograd, name, batch, train, relu)


def dx(cls, winograd, name, batch, masked=True, has_addend=False, want_bias=False):
    cin, _, k, _ = SHAPES[cls][name]
    if k == 5:
        return routes.convT_dx(cls, winograd, name, cin, batch)
    return routes.conv_dx(cls, winograd, name, batch, masked, has_addend, want_bias)


# (class, winograd) -> layer -> (training forward, evaluation forward, backward-data of a training step) at 16, 64, 65 and
# 917 blocks; one string: the same at all four.  The backward-data is what _bwd_trunk asks for: through the ReLU mask,
# and with a use for the bias slabs where the five-gradient launch runs (the narrow decoder).
AT = (16, 64, 65, 917)
G, T = "gather", "convT_fwd"
TABLES = {
    ("narrow", True): {
        "up0": (T, T, G),
        "conv0": (T, T, G),
        "up1": ("convT_mfma v15", "convT_mfma v5", ("s2k5_mfma v7", "s2k5_mfma v7", "s2k5_mfma v2", "s2k5_mfma v2")),
        "conv1": (("k4_mfma", "k4_mfma v5", "wino_fwd ppc8", "wino_fwd ppc8"),
                  ("k4_mfma", "k4_mfma v5", "k4_mfma v5", "k4_mfma v5"),
                  ("wino_bwd +slabs", "wino_bwd +slabs", "wino_bwd ppc10", "wino_bwd ppc10")),
        "up2": ("convT_mfma v15", "convT_mfma v5", ("s2k5_mfma v6", "s2k5_mfma v6", "s2k5_mfma v5", "s2k5_mfma v5")),
        "conv2": (("wino_fwd", "wino_fwd", "wino_fwd ppc16", "wino_fwd ppc16"),
                  "k4_mfma",
                  ("wino_bwd +slabs", "wino_bwd +slabs", "wino_bwd ppc18", "wino_bwd ppc18")),
    },
    ("narrow", False): {
        "up0": (T, T, G),
        "conv0": (T, T, G),
        "up1": ("convT_mfma v5", "convT_mfma v5", ("s2k5_mfma", "s2k5_mfma", "s2k5_mfma v2", "s2k5_mfma v2")),
        "conv1": (("k4_mfma", "k4_mfma v5", "k4_mfma v5", "k4_mfma v5"),
                  ("k4_mfma", "k4_mfma v5", "k4_mfma v5", "k4_mfma v5"),
                  ("k4_mfma +slabs", "k4_mfma +slabs", G, G)),
        "up2": ("convT_mfma v5", "convT_mfma v5", ("s2k5_mfma v6", "s2k5_mfma v6", "s2k5_mfma v5", "s2k5_mfma v5")),
        "conv2": ("k4_mfma", "k4_mfma", ("k4_mfma +slabs", "k4_mfma +slabs", G, G)),
    },
    ("wide", True): {
        "up0": ("convT16", "convT16", "g16"),
        "conv0": ("convT16", "convT16", "g16"),
        "up1": ("convT16", "convT16", "g16"),
        "conv1": ("g16", "g16", "wino16_bwd"),          # never a Winograd forward
        "up2": ("convT16", "convT16", "g16"),
        "conv2": ("wino16_fwd", "g16", "wino16_bwd"),
    },
    ("wide", False): {name: (("g16", "g16", "g16") if name.startswith("conv") and name != "conv0" else
                             ("convT16", "convT16", "g16")) for name in TRUNK},
}


def test_the_route_tables():
    for (cls, winograd), table in TABLES.items():
        assert tuple(table) == TRUNK
        for name, columns in table.items():
            want = [(c,) * len(AT) if isinstance(c, str) else c for c in columns]
            got = [tuple(show(fwd(cls, winograd, name, b, True)) for b in AT),
                   tuple(show(fwd(cls, winograd, name, b, False)) for b in AT),
                   tuple(show(dx(cls, winograd, name, b, want_bias=cls == "narrow")) for b in AT)]
            assert got == want, (cls, winograd, name)
    # the packings behind them
    assert routes.conv_fwd("narrow", True, "conv1", 65, True, True).pack == "wino_fwd"
    assert routes.conv_fwd("narrow", True, "conv1", 64, True, True).pack == "k4_fwd"
    assert routes.convT_fwd("narrow", True, "up2", 8, True).pack == "convT_rows"
    assert routes.convT_fwd("narrow", True, "up2", 8, False).pack == "convT"
    assert routes.conv_dx("narrow", False, "conv1", 16, True, False, True).pack == "k4_dx_z"
    assert routes.conv_dx("narrow", False, "conv2", 16, True, False, True).pack == "k4_dx_x"
    assert (routes.PAIR_AXIS["k4_dx_z"], routes.PAIR_AXIS["k4_dx_x"]) == (2, 0)
    # the heads' share arrives as an addend in no trunk convolution, and the Winograd kernels take none
    assert show(routes.conv_dx("narrow", True, "conv2", 16, True, True, True)) == "k4_mfma"
    assert show(routes.conv_dx("wide", True, "conv2", 16, True, True, False)) == "g16"
    # weight gradients outside the one-launch groupings: the wide decoder's Winograd form, conv2 whole, conv1 split in z
    assert routes.conv_wgrad("wide", True, "conv2") == routes.WgradRoute("wino16_partial", 0)
    assert routes.conv_wgrad("wide", True, "conv1") == routes.WgradRoute("wino16_partial", 8)
    assert all(routes.conv_wgrad(cls, w, name) == routes.WgradRoute("tiled", 0)
               for cls, w in (("wide", False), ("narrow", True), ("generic", True)) for name in SHAPES[cls])
    assert routes.BATCH_SWITCH == 64
    # the wide up0's matrix-core kernels exist for 8 latent channels only
    assert routes.layer_packs("wide", True, "up0", 8, 16, 5, 2) == ("g16_dx", "convT16")
    for ch in (3, 4, 16):
        assert routes.layer_packs("wide", True, "up0", ch, 16, 5, 2) == ()
        assert show(routes.convT_fwd("wide", True, "up0", ch, True)) == T and show(routes.convT_dx("wide", True, "up0", ch, 16)) == G


def reorders(r):
    """The route takes a form with another summation order than the direct kernels."""
    return r.form in routes.WINOGRAD_FORMS or (r.form, r.variant) in routes.REORDERING_VARIANTS


def test_every_route_keeps_the_contract():
    assert set(routes.REORDERING_VARIANTS) == {("convT_mfma", 15), ("s2k5_mfma", 7)}
    for cls, winograd in itertools.product(CLASSES, (True, False)):
        for name, (cin, cout, k, pad) in SHAPES[cls].items():
            held = routes.layer_packs(cls, winograd, name, cin, cout, k, pad)
            assert set(held) <= set(routes.PACKS) and (cls != "generic" or held == ())
            found = []
            for train in (True, False):
                forms = set()
                for batch, relu in itertools.product(BATCHES, (True, False)):
                    r = fwd(cls, winograd, name, batch, train, relu)
                    found.append(((batch, train, relu), r))
                    assert not r.bias_slabs
                    if not train or not winograd:
                        assert not reorders(r), (cls, winograd, name, batch, train, r)
                    if not train:
                        forms.add((relu, r.form, r.pack))
                # an evaluation forward: the form does not depend on the batch, only the variant may
                assert train or len(forms) == 2, (cls, winograd, name, forms)
            for batch, masked, addend, want_bias in itertools.product(BATCHES, *[(True, False)] * 3):
                r = dx(cls, winograd, name, batch, masked, addend, want_bias)
                found.append(((batch, masked, addend, want_bias), r))
                assert winograd or not reorders(r), (cls, name, batch, r)
                assert not r.bias_slabs or (masked and not addend and want_bias), (cls, winograd, name, batch, r)
            if k != 5:
                w = routes.conv_wgrad(cls, winograd, name)
                assert w.form in ("tiled", "wino16_partial") and (winograd or w.form == "tiled")
                assert cls != "generic" or w.form == "tiled"
            for what, r in found:
                what = (cls, winograd, name) + what + (r,)
                # a route reads a packing the layer holds, or none: the shape-generic forms
                assert (r.pack is None) == (r.form in routes.GENERIC_FORMS), what
                assert r.pack is None or r.pack in held, what
                assert cls != "generic" or r.form in routes.GENERIC_FORMS, what
                assert r.form != "k4_mfma" or r.pack in routes.PAIR_AXIS, what


def test_pack_jobs_fit_the_one_launch():
    """nvf_pack_mfma_all / nvf_step_head take at most 16 jobs (pack_jobs_desc, csrc/pack_mfma.h)."""
    count = {}
    for cls, winograd in itertools.product(CLASSES, (True, False)):
        jobs = [(p, name) + routes.pack_job(p, cin, cout, k) for p in routes.PACKS
                for name, (cin, cout, k, pad) in SHAPES[cls].items()
                if p in routes.layer_packs(cls, winograd, name, cin, cout, k, pad)]
        assert len(jobs) <= 16
        assert all(c0 > 0 and c0 % 4 == 0 for _, _, _, c0, _ in jobs)
        count[cls, winograd] = len(jobs)
        if (cls, winograd) == ("narrow", True):
            # packing by packing, layers in table order: the job order of the step head
            assert jobs == [("k4_fwd", "conv1", 0, 8, 8), ("k4_fwd", "conv2", 0, 8, 8), ("k4_dx_z", "conv1", 2, 8, 8),
                            ("k4_dx_x", "conv2", 0, 8, 8), ("wino_dx", "conv1", 40, 8, 8), ("wino_dx", "conv2", 40, 8, 8),
                            ("wino_fwd", "conv1", 40, 8, 8), ("wino_fwd", "conv2", 40, 8, 8), ("convT", "up1", 10, 16, 8),
                            ("convT", "up2", 10, 8, 8), ("convT_rows", "up1", 12, 16, 8), ("convT_rows", "up2", 12, 8, 8),
                            ("s2k5_dx", "up1", 20, 8, 16), ("s2k5_dx", "up2", 20, 8, 8)]
        if (cls, winograd) == ("wide", True):
            assert jobs == [("wino16_dx", "conv1", 41, 16, 16), ("wino16_dx", "conv2", 41, 16, 16),
                            ("wino16_fwd", "conv2", 41, 16, 16), ("g16_fwd", "conv1", 30, 16, 16),
                            ("g16_fwd", "conv2", 30, 16, 16), ("g16_dx", "up0", 31, 16, 8), ("g16_dx", "conv0", 31, 32, 16),
                            ("g16_dx", "up1", 31, 16, 32), ("g16_dx", "conv1", 30, 16, 16), ("g16_dx", "up2", 31, 16, 16),
                            ("g16_dx", "conv2", 30, 16, 16), ("convT16", "up0", 11, 8, 16), ("convT16", "conv0", 11, 16, 32),
                            ("convT16", "up1", 11, 32, 16), ("convT16", "up2", 11, 16, 16)]
    assert count == {("narrow", True): 14, ("narrow", False): 8, ("wide", True): 15, ("wide", False): 12,
                     ("generic", True): 0, ("generic", False): 0}
    # kind 12 has no nvf_pack_*_floats: (cin / 4) x 65 fragments of 64 floats, as pack_jobs_desc sizes it
    assert routes.pack_floats(None, "convT_rows", 16, 8, 5) == 4 * 65 * 64
