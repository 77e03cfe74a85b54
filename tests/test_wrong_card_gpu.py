"""A tensor on another card than the model's is refused by every ``HipEngine`` method before anything is launched: a kernel on
card A must never get a pointer into card B (``HipEngine._tensors``).  Needs two visible cards."""
import pytest

pytestmark = pytest.mark.gpu


def test_tensor_on_another_card_is_refused_before_any_launch(ckpt_weights):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible card")
    from catfish_amd.engine import HipEngine
    engine = HipEngine(ckpt_weights, device=0, max_windows_per_pass=64)
    try:
        probs = torch.zeros(35, dtype=torch.float32, device="cuda:1")
        dac = torch.zeros(35, dtype=torch.int16, device="cuda:1")
        offsets = torch.tensor([0, 35], dtype=torch.int64, device="cuda:0")
        lengths = torch.tensor([35], dtype=torch.int64, device="cuda:0")
        with pytest.raises(ValueError, match="postprocess_device: probs lives on cuda:1, model on cuda:0"):
            engine.postprocess_device(probs, offsets, lengths)
        with pytest.raises(ValueError, match="normalize_device: dac lives on cuda:1, model on cuda:0"):
            engine.normalize_device(dac, offsets, offsets)
        with pytest.raises(ValueError, match="vote_device: probs_all lives on cuda:1, model on cuda:0"):
            engine.vote_device(probs, offsets, lengths, 35, (0,))
        # the tables on the other card, the samples on the model's
        with pytest.raises(ValueError, match="postprocess_device: read_offsets lives on cuda:1"):
            engine.postprocess_device(probs.to("cuda:0"), offsets.to("cuda:1"), lengths)
        with pytest.raises(ValueError, match="vote_device: lengths lives on cuda:1"):
            engine.vote_device(probs.to("cuda:0"), offsets, lengths.to("cuda:1"), 35, (0,))
        torch.cuda.synchronize(0)
        engine.check_error()
    finally:
        engine.close()
