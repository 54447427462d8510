"""GPU: the staged device-to-host copies of SequenceOutputs with every route on at once (tests/sequence_all_routes_cases.py): the tree
written from device tensors is, byte for byte and manifest included, the tree written from the same host arrays.  No kernel of the
project is launched."""
import pytest

import sequence_all_routes_cases as A

pytestmark = pytest.mark.gpu


def test_device_tensors_write_the_tree_of_the_host_arrays(tmp_path):
    A.run(tmp_path / "host").close()
    A.run(tmp_path / "device", to=lambda t: t.cuda()).close()
    host, device = A.tree(tmp_path / "host"), A.tree(tmp_path / "device")
    assert sorted(device) == sorted(host) and len(host) == 6 * len(A.NAMES) + 2
    assert [k for k in host if device[k] != host[k]] == []
