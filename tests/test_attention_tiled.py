"""vit_b_16: the model the tiled attention kernels were built for."""

import pytest

from mi355x_ddp.models import vit_b_16


@pytest.fixture(scope="module")
def torch_model():
    return vit_b_16()


def test_vit_b_16_has_torchvisions_parameter_count(torch_model):
    hidden, mlp, layers, classes, patch = 768, 3072, 12, 1000, 16
    tokens = (224 // patch) ** 2 + 1
    assert tokens == 197
    block = (2 * 2 * hidden                          # ln_1, ln_2
             + 3 * hidden * hidden + 3 * hidden      # in-projection
             + hidden * hidden + hidden              # out-projection
             + 2 * hidden * mlp + mlp + hidden)      # MLP
    want = (3 * patch * patch * hidden + hidden      # conv_proj
            + hidden + tokens * hidden               # class token, positions
            + layers * block + 2 * hidden            # encoder, final ln
            + hidden * classes + classes)            # head
    assert want == 86_567_656  # torchvision's published count
    assert sum(p.numel() for p in torch_model.parameters()) == want


def test_vit_b_16_state_dict_names_do_not_depend_on_attention(torch_model):
    hip = vit_b_16(attention="hip").state_dict()
    assert list(hip) == list(torch_model.state_dict())
    assert all(hip[k].shape == v.shape
               for k, v in torch_model.state_dict().items())
