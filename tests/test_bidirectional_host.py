"""RAFT.forward_bidirectional without a GPU: the signature and the argument check that needs no kernel (the forward
itself runs on the GPU only: tests/test_gpu_bidirectional.py)."""
import pytest
import torch

from model import RAFT


def test_flow_init_pair_is_validated_before_any_work():
    model = RAFT().eval()
    img = torch.zeros(1, 3, 128, 160)
    with pytest.raises(TypeError, match="pair"):
        model.forward_bidirectional(img, img, iters=1, flow_init=torch.zeros(1, 2, 16, 20))
    with pytest.raises(TypeError, match="pair"):
        model.forward_bidirectional(img, img, iters=1, flow_init=(None, None, None))


def test_method_exists_with_the_documented_signature():
    import inspect

    sig = inspect.signature(RAFT.forward_bidirectional)
    assert list(sig.parameters) == ["self", "image0", "image1", "iters", "flow_init", "test_mode"]
    assert sig.parameters["iters"].default == 12 and sig.parameters["flow_init"].default is None
    assert sig.parameters["test_mode"].default is False
