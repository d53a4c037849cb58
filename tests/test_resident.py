"""analysisgnn_amd/resident.py without a device: CPU tensors stand in for device buffers, and the one function through which the
registry asks whether the current stream is capturing is replaced.  The keys, what a capture may and may not leave cached, the
alignment and growth of scratch, and the FIFO bound of the `ones` family."""
import pytest
import torch


@pytest.fixture
def resident(monkeypatch):
    from analysisgnn_amd import resident as r
    for name in ("_STREAMS", "_VALUES", "_SCRATCH"):            # an empty registry for the test, the process's own back afterwards
        monkeypatch.setattr(r, name, {})
    return r


def test_short_and_indexed_spellings_are_one_key(resident, monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    r = resident
    assert r.device_index("cuda") == r.device_index("cuda:0") == r.device_index(torch.device("cuda", 0)) == r.device_index(0) == 0
    assert r.device_index(torch.device("cuda")) == 0 and r.device_index("cuda:3") == 3
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 2)
    assert r.device_index("cuda") == 2
    made = []
    monkeypatch.setattr(r, "_capturing", lambda idx: False)
    a = r.value("cuda", ("unit gradient",), lambda: made.append(1) or torch.ones(()))
    b = r.value(torch.device("cuda", 2), ("unit gradient",), lambda: made.append(1) or torch.ones(()))
    assert a is b and len(made) == 1 and list(r._VALUES) == [(2, ("unit gradient",))]


def test_the_cpu_is_never_asked_about_captures(resident, monkeypatch):
    def boom():
        raise AssertionError("asked the HIP runtime about a CPU device")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", boom)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: boom())
    assert resident.lane("cpu") == "main"
    assert resident.value("cpu", ("offset table", (0, 4)), lambda: torch.tensor([0, 4])).tolist() == [0, 4]
    assert resident.scratch("cpu", "t", 16, True).numel() == 16


def test_missing_value_under_capture_raises_and_caches_nothing(resident, monkeypatch):
    from analysisgnn_amd._lib import AgnnError
    monkeypatch.setattr(resident, "_capturing", lambda idx: True)
    made = []
    with pytest.raises(AgnnError, match="offset table.*before a hipGraph capture starts.*eagerly"):
        resident.value("cpu", ("offset table", (0, 4, 9)), lambda: made.append(1))
    assert not made and not resident._VALUES                       # refused before anything was built
    ones = resident.value("cpu", ("ones", (2, 3)), lambda: torch.ones(2, 3), fill=True)     # a plain fill: handed out, not kept
    assert torch.equal(ones, torch.ones(2, 3)) and not resident._VALUES
    monkeypatch.setattr(resident, "_capturing", lambda idx: False)
    t = resident.value("cpu", ("offset table", (0, 4, 9)), lambda: torch.tensor([0, 4, 9]))
    monkeypatch.setattr(resident, "_capturing", lambda idx: True)
    assert resident.value("cpu", ("offset table", (0, 4, 9)), lambda: made.append(1)) is t and not made   # present: served under capture


def test_scratch_under_capture_is_handed_out_but_not_cached(resident, monkeypatch):
    monkeypatch.setattr(resident, "_capturing", lambda idx: True)
    for nbytes in (1, 8464, 100_001):
        buf = resident.scratch("cpu", "ticket", nbytes, zeroed=True)
        assert buf.dtype == torch.uint8 and buf.numel() == nbytes and buf.data_ptr() % 256 == 0
        assert int(buf.count_nonzero()) == 0
        assert not resident._SCRATCH
    monkeypatch.setattr(resident, "_capturing", lambda idx: False)
    small = resident.scratch("cpu", "ticket", 64, zeroed=True)
    monkeypatch.setattr(resident, "_capturing", lambda idx: True)
    assert resident.scratch("cpu", "ticket", 64, zeroed=True) is small         # large enough: the cached one, also under capture
    big = resident.scratch("cpu", "ticket", 4096, zeroed=True)                 # too small: a buffer of this capture's own ...
    assert big is not small and big.numel() == 4096 and big.data_ptr() % 256 == 0
    assert list(resident._SCRATCH.values()) == [small] and resident._SCRATCH[(-1, "main", "ticket")] is small   # ... and no replacement


def test_scratch_outside_a_capture_is_cached_and_grows(resident, monkeypatch):
    monkeypatch.setattr(resident, "_capturing", lambda idx: False)
    a = resident.scratch("cpu", "ws", 1000, zeroed=False)
    assert a.data_ptr() % 256 == 0 and a.numel() == 1000
    assert resident.scratch("cpu", "ws", 1000, zeroed=False) is a
    assert resident.scratch("cpu", "ws", 10, zeroed=False) is a                # a smaller request is served by the same buffer
    b = resident.scratch("cpu", "ws", 5000, zeroed=False)
    assert b is not a and b.numel() == 5000 and b.data_ptr() % 256 == 0
    assert resident.scratch("cpu", "ws", 1000, zeroed=False) is b and len(resident._SCRATCH) == 1
    assert resident.scratch("cpu", "other", 8, zeroed=True) is not b and len(resident._SCRATCH) == 2    # one per name


def test_ones_family_keeps_the_newest_eight(resident, monkeypatch):
    monkeypatch.setattr(resident, "_capturing", lambda idx: False)
    assert resident.FIFO == {"ones": 8}
    first = [resident.value("cpu", ("ones", (n,)), lambda n=n: torch.ones(n)) for n in range(1, 9)]
    table = resident.value("cpu", ("index table", (1, 2)), lambda: torch.tensor([1, 2]))
    assert resident.value("cpu", ("ones", (1,)), lambda: None) is first[0] and len(resident._VALUES) == 9      # eight: all kept
    resident.value("cpu", ("ones", (9,)), lambda: torch.ones(9))                                                # the ninth evicts the oldest
    keys = [k[1] for k in resident._VALUES if k[1][0] == "ones"]
    assert keys == [("ones", (n,)) for n in range(2, 10)]
    assert resident.value("cpu", ("ones", (2,)), lambda: None) is first[1]
    assert resident.value("cpu", ("index table", (1, 2)), lambda: None) is table                                # other families: unbounded, untouched
