"""`basecall` over several devices without a GPU: the group planner — po_basecall_group_plan through the
library, which loads without a device, and its Python restatement — and the command's refusals that come before any
device work."""
import numpy as np
import pytest


def _lib_plan(lens, group_samples, ndev=1):
    from poreover_amd import _lib
    lib = _lib.load(require_gpu=False)
    a = np.ascontiguousarray(lens, dtype=np.int64)
    first = np.zeros(max(len(a), 1), dtype=np.int32)
    count = np.zeros(max(len(a), 1), dtype=np.int32)
    g = lib.po_basecall_group_plan(a.ctypes.data, len(a), int(group_samples), ndev, first.ctypes.data, count.ctypes.data, len(a))
    assert g >= 0
    return [(int(first[i]), int(count[i])) for i in range(g)]


def _check(lens, cap, groups):
    at = 0
    for f, c in groups:                       # every read in exactly one group, in order
        assert f == at and c >= 1
        at += c
        assert sum(lens[f:f + c]) <= cap or c == 1          # over the cap only as a single read
        if f + c < len(lens):                               # greedy: the next read would not have fitted
            assert sum(lens[f:f + c + 1]) > cap
    assert at == len(lens)


@pytest.mark.parametrize("ndev", range(1, 17))
def test_groups_of_a_ragged_batch(ndev):
    from poreover_amd.network import basecall as B
    rng = np.random.default_rng(ndev)
    lens = [int(x) for x in rng.integers(1, 9000, 200)]
    giant = list(lens)
    giant[17] = 4000000                                       # longer than any cap below: it goes alone
    for budget, lens in ((10 ** 12, lens), (50000, lens), (7, lens), (10 ** 12, giant), (50000, giant)):
        gs = B.group_samples(sum(lens), budget, ndev)
        from poreover_amd import _lib
        assert gs == _lib.load(require_gpu=False).po_basecall_group_samples(sum(lens), budget, ndev)
        assert gs == max(1, min(budget, -(-sum(lens) // (2 * ndev))))
        groups = B.group_plan(lens, gs)
        assert groups == _lib_plan(lens, gs, ndev)
        _check(lens, gs, groups)
        if lens is giant:
            assert (17, 1) in groups and gs < giant[17]
        else:
            assert len(groups) >= 2 * ndev                    # 200 reads, none above a share: the reads allow it


def test_edges():
    from poreover_amd.network import basecall as B
    assert B.group_plan([], 10) == _lib_plan([], 10) == []
    assert B.group_plan([5], 10) == _lib_plan([5], 10) == [(0, 1)]
    assert B.group_plan([50], 10) == _lib_plan([50], 10) == [(0, 1)]
    assert B.group_plan([4, 6, 1, 30, 2, 2], 10) == _lib_plan([4, 6, 1, 30, 2, 2], 10) == [(0, 2), (2, 1), (3, 1), (4, 2)]
    assert B.group_samples(0, 100, 4) == 1 and B.group_samples(10, 100, 1) == 5 and B.group_samples(1000, 100, 2) == 100
    from poreover_amd import _lib
    lib = _lib.load(require_gpu=False)
    assert lib.po_basecall_group_plan(None, 0, 0, 1, None, None, 0) == _lib.E_ARG
    assert b"group_samples 0" in lib.po_last_error()
    a = np.array([3, 3, 3], dtype=np.int64)                   # a table shorter than the groups: counted, not written
    first = np.full(1, -1, dtype=np.int32)
    count = np.full(1, -1, dtype=np.int32)
    assert lib.po_basecall_group_plan(a.ctypes.data, 3, 3, 1, first.ctypes.data, count.ctypes.data, 1) == 3
    assert (first[0], count[0]) == (0, 1)


def _parse(argv):
    from poreover_amd.__main__ import build_parser
    return build_parser().parse_args(argv)


def test_parser():
    a = _parse(["basecall", "reads", "--weights", "w.npz"])
    assert a.gpus is None and a.readers == 4 and a.chunk_files is None
    a = _parse(["basecall", "reads", "--weights", "w.npz", "--gpus", "0", "--readers", "16", "--chunk_files", "1"])
    assert (a.gpus, a.readers, a.chunk_files) == (0, 16, 1)


@pytest.mark.parametrize("readers", (0, 17, -1))
def test_readers_outside_1_to_16_is_refused(readers, tmp_path):
    from poreover_amd.network import basecall as B
    a = _parse(["basecall", str(tmp_path), "--weights", str(tmp_path / "none.npz"), "--gpus", "1", "--readers", str(readers)])
    with pytest.raises(SystemExit, match=r"--readers %d must be 1 to 16" % readers):
        B.basecall(a)


def test_gpus_above_the_count_is_refused(tmp_path, monkeypatch):
    from poreover_amd import _lib
    from poreover_amd.network import basecall as B

    class Two:
        @staticmethod
        def po_device_count():
            return 2
    monkeypatch.setattr(_lib, "load", lambda require_gpu=True: Two)
    assert B.stream_devices(2) == [0, 1] and B.stream_devices(0) == [0, 1] and B.stream_devices(1) == [0]
    a = _parse(["basecall", str(tmp_path), "--weights", str(tmp_path / "none.npz"), "--gpus", "3"])
    with pytest.raises(SystemExit, match="basecall: --gpus 3, but 2 devices are visible"):
        B.basecall(a)
    Two.po_device_count = staticmethod(lambda: 1)
    with pytest.raises(SystemExit, match="basecall: --gpus 2, but 1 device is visible"):
        B.stream_devices(2)
    with pytest.raises(SystemExit, match="--gpus must not be negative"):
        B.stream_devices(-1)
