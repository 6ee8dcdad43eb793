"""The caller-written inputs of DDPEngine on the GPU, every row of ``ddp_amd.engine.CALLER_INPUTS`` on every task it exists for, through
the public methods of its name: clear value after construction, exact bytes after ``set_*``, cleared by ``set_geometry`` there and back,
view and output after ``SampleGraph.replay(<name>=v)`` (tests/conditioning_cases.py has the checks).  Needs an MI355X: ``pytest -m gpu``.
(CPU companion: tests/test_conditioning_host.py; what each input does to the output is the subject of test_x0_hints_gpu /
test_prior_start_gpu / test_class_prior_gpu / test_score_prior_gpu.)

One test for the seven (input, task) pairs, about a third of a second each: every pair runs whatever the others did, and the failure
names each pair that failed."""
import traceback

import pytest

import conditioning_cases as CC
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def test_view_set_clear_and_replay(dev):
    assert CC.PAIRS == [('score_prior', 'seg'), ('class_prior', 'seg'), ('prior', 'seg'), ('prior', 'depth'), ('prior', 'bev'),
                        ('hints', 'seg'), ('hints', 'depth')]
    failed = {}
    for name, task in CC.PAIRS:
        try:
            CC.check(dev, name, task)
        except AssertionError:                       # (a missed check; any other error, a device's included, ends the test there)
            failed[f'{name}-{task}'] = traceback.format_exc()
    assert not failed, '\n'.join(f'---- {pair} ----\n{tb}' for pair, tb in failed.items())
