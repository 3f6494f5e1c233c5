"""CPU tier: the host-side mirror of the reference API (validation, broadcasting, early exits, padding, dtype
rules, composition chains), with the three native primitives served by the CPU oracle, must reproduce every
golden case the reference produced -- bit for bit, values and masks.  Where a 3 x 3 matrix comes out of host
linear algebra on the way, the fixtures' host's matrix is replayed (tests/golden/host_algebra.py): this host's
own must agree with it to fp32 rounding."""
import pytest
import torch

from conftest import golden_ids
import case_runner
import host_algebra

ALL = [c for c in golden_ids() if not c.endswith("cfg1_inputs") and not c.startswith("grads.")]   # (gradients: GPU tier, the oracle is forward-only)


@pytest.mark.parametrize("cid", ALL)
def test_golden_case_cpu(cid, golden, oracle_native, monkeypatch):
    case = golden.cases[cid]
    replayed = host_algebra.pin(cid, monkeypatch)
    got = case_runner.run_case(case, golden, torch.device('cpu'))
    case_runner.check_case(case, golden, got, exact_values=True)
    replayed()
