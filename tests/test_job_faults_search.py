"""The poked cells of tests/test_gpu_job_faults.py are what its seeded search finds on the honest host traces (no GPU):
`python -m tests.test_gpu_job_faults --search` prints the same tables."""
import pytest

from tests import test_gpu_job_faults as F


def test_the_three_shard_cells_are_the_searchs():
    assert F.search_job3() == F.JOB3


@pytest.mark.parametrize("name", list(F.GUESTS))
def test_the_guest_cells_are_the_searchs(name):
    assert F.search_guest(name) == F.GUEST_CELLS[name]
    assert all(cell is not None for cell in F.GUEST_CELLS[name].values())


def test_every_chip_but_cpu_is_poked_in_some_guest():
    assert set(F.GUEST_CELLS) == set(F.GUESTS)
    assert sorted({c for cells in F.GUEST_CELLS.values() for c in cells}) == [0, 1] + list(range(3, 14))
