"""The drop-in case of tests/test_host.py::test_dropin_through_reference_registry_and_detector: detector config, seeded weights and
inputs, reproducible from names and shapes alone, so that the golden fixture (recorded from the reference's own YoloXDetector by
oracle/make_golden_dropin.py) stores only the state_dict names, its integer buffers and the reference's outputs."""
import zlib

import torch

GOLDEN = 'dropin_detector'


def model_cfg(impl=None):
    """The detector config of the case (the reference's YoloXDetector layout).  `impl` is the key the registry branches of
    INTEGRATION.md sections 1, 5 and 6 read ('mi355x': rvt_amd); None leaves it out, as the unmodified reference expects."""
    cfg = {
        'backbone': {'name': 'MaxViTRNN', 'impl': impl, 'compile': {'enable': False, 'args': {'mode': 'reduce-overhead'}},
                     'input_channels': 20, 'enable_masking': False, 'partition_split_32': 1, 'embed_dim': 32,
                     'dim_multiplier': [1, 2, 4, 8], 'num_blocks': [1, 1, 1, 1], 'T_max_chrono_init': [4, 8, 16, 32],
                     'stem': {'patch_size': 4}, 'in_res_hw': [64, 96],
                     'stage': {'downsample': {'type': 'patch', 'overlap': True, 'norm_affine': True},
                               'attention': {'use_torch_mha': False, 'partition_size': [2, 3], 'dim_head': 32,
                                             'attention_bias': True, 'mlp_activation': 'gelu', 'mlp_gated': False,
                                             'mlp_bias': True, 'mlp_ratio': 4, 'drop_mlp': 0, 'drop_path': 0,
                                             'ls_init_value': 1e-5},
                               'lstm': {'dws_conv': False, 'dws_conv_only_hidden': True, 'dws_conv_kernel_size': 3,
                                        'drop_cell_update': 0}}},
        'fpn': {'name': 'PAFPN', 'impl': impl, 'compile': {'enable': False, 'args': {'mode': 'reduce-overhead'}}, 'depth': 0.67,
                'in_stages': [2, 3, 4], 'depthwise': False, 'act': 'silu'},
        'head': {'name': 'YoloX', 'impl': impl, 'compile': {'enable': False, 'args': {'mode': 'reduce-overhead'}}, 'depthwise': False,
                 'act': 'silu', 'num_classes': 3},
    }
    for part in cfg.values():
        if impl is None:
            del part['impl']
    return cfg


def seeded_value(name, like):
    """A floating state_dict entry as a function of its name and shape: weights ~ N(0, 1 / fan_in), norm scales and LayerScale
    gammas near 1 / in [0.5, 1.5) (1e-5 would hide the attention / MLP branches), BatchNorm statistics positive variances."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    shape, leaf = tuple(like.shape), name.rsplit('.', 1)[-1]
    if leaf == 'gamma':
        v = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
    elif leaf == 'running_var':
        v = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
    elif len(shape) >= 2:
        fan_in = 1
        for d in shape[1:]:
            fan_in *= d
        v = torch.randn(shape, generator=g, dtype=torch.float64) / fan_in ** 0.5
    elif leaf == 'weight':
        v = 1.0 + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
    else:                                   # biases, running means, other vectors
        v = 0.05 * torch.randn(shape, generator=g, dtype=torch.float64)
    return v.to(like.dtype)


def seeded_state(template, int_buffers):
    """The case's state_dict for a module whose state_dict() is `template`: floating entries from seeded_value, integer buffers
    from `int_buffers` (name -> tensor, as recorded from the reference)."""
    out = {}
    for n, t in template.items():
        out[n] = seeded_value(n, t) if t.is_floating_point() else torch.as_tensor(int_buffers[n]).to(t.dtype).reshape(t.shape)
    return out


def make_inputs():
    """(T=3, B=2, 20, 60, 90) uint8 event tensors (padded to 64 x 96 by the caller, modules/detection.py:133-134)."""
    return torch.randint(0, 11, (3, 2, 20, 60, 90), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)


def make_targets():
    targets = torch.zeros(2, 4, 5)
    targets[0, 0] = torch.tensor([1., 30., 20., 24., 18.])
    targets[0, 1] = torch.tensor([0., 70., 44., 30., 28.])
    targets[1, 0] = torch.tensor([2., 50., 30., 60., 40.])
    return targets
