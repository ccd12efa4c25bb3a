"""Argument checks of ops.conv_wino_bn's channel form (bn_axis=1) and of the coefficient shape
both axes now check: every case raises ValueError in Python, before the native library is
touched, so these run on CPU tensors without a GPU."""
import pytest
import torch

from rocalphago_amd.ops import hipops as ops

B, S, C = 2, 19, 128


def operands():
    x = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16)
    y = torch.zeros_like(x)
    u = torch.zeros(12, C, C, dtype=torch.bfloat16)
    return x, u, torch.zeros(C), y


def call(**kw):
    x, u, b, y = operands()
    return ops.conv_wino_bn(x, u, b, y, B, S, C, C, False, **kw)


@pytest.mark.parametrize("shape", [(3, S), (2, C), (3, C + 1), (3 * C,), (1, 3, C)])
def test_channel_form_refuses_wrong_coef_shape(shape):
    with pytest.raises(ValueError):
        call(bn_coef=torch.zeros(shape), bn_axis=1)


def test_channel_form_refuses_wrong_coef_dtype_and_missing_coef():
    with pytest.raises(ValueError):
        call(bn_coef=torch.zeros(3, C, dtype=torch.float64), bn_axis=1)
    with pytest.raises(ValueError):
        call(bn_axis=1)


@pytest.mark.parametrize("shape", [(B - 1, 2, C), (B, 2, S), (B, 3, C), (B, 2 * C), (B, 2, C + 8)])
def test_channel_form_refuses_wrong_stat_part_shape(shape):
    with pytest.raises(ValueError):
        call(bn_coef=torch.zeros(3, C), stat_part=torch.zeros(shape), bn_axis=1)


def test_channel_form_is_forward_only():
    coef = torch.zeros(3, C)
    x = operands()[0]
    with pytest.raises(ValueError):
        call(bn_coef=coef, mask_coef=coef, bn_axis=1)
    with pytest.raises(ValueError):
        call(mask=x, mask_coef=coef, bn_axis=1)
    with pytest.raises(ValueError):
        call(bn_coef=coef, mask=x, bn_axis=1)
    with pytest.raises(ValueError):
        call(bn_coef=coef, stat_mean=torch.zeros(C), bn_axis=1)
    with pytest.raises(ValueError):
        call(bn_coef=coef, bn_axis=0)


@pytest.mark.parametrize("shape", [(3, C), (2, S), (3, S + 1)])
def test_column_form_checks_its_coef_shape(shape):
    with pytest.raises(ValueError):
        call(bn_coef=torch.zeros(shape))
