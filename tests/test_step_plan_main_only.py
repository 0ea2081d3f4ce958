"""The main-head-only form of engine.plan_step (latent passes under a frozen decoder), without a device: it is the
latent pass's plan with the heads' entry replaced, it exists for every decoder class and batch, and it is refused for a
pass with weight gradients.  tests/test_step_plan.py holds the default form."""
import itertools

import pytest

from nvfpcc_amd.engine import plan_step
from tests.test_step_plan import CLASSES, SWITCHES


def latent_plan(cls, batch, naive=0, winograd=True, **kw):
    c = CLASSES[cls]
    tuned_class = cls != "generic"
    return plan_step(c["narrow"], c["wide"], winograd, tuned_class and c["ch"] <= 8, True, tuned_class, c["ch"], batch,
                     False, True, False, False, naive, *[True] * len(SWITCHES), **kw)


def test_main_only_changes_the_heads_entry_alone():
    for cls, batch, naive, wino in itertools.product(CLASSES, (1, 12, 32, 33, 64, 65, 917, 4096), (0, 1), (True, False)):
        base, main = latent_plan(cls, batch, naive, wino), latent_plan(cls, batch, naive, wino, main_only=True)
        assert base.heads in ("fused_loss", "heads3", "layers") and main.heads == "main", (cls, batch, naive)
        assert main == base._replace(heads="main"), (cls, batch, naive)
        assert not (main.want_w or main.head_bias_in_loss or main.heads_in_trunk5 or main.trunk5 or main.tail_queued)
        assert latent_plan(cls, batch, naive, wino, main_only=False) == base


def test_main_only_is_refused_with_weight_gradients():
    c = CLASSES["narrow"]
    for want_emb in (False, True):
        with pytest.raises(ValueError, match="main_only"):
            plan_step(c["narrow"], c["wide"], True, True, True, True, c["ch"], 16, True, want_emb, False, False, 0,
                      *[True] * len(SWITCHES), main_only=True)
