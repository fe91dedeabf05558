"""uint8 pixels in front of an image stem: normalisation as one float32 table.

A decoded image is HWC bytes -- this library's NHWC layout.  ToTensor() + Normalize(mean, std) (the reference's loaders,
utils/preprocessing.py:4-35), like any per-channel elementwise preprocessing, maps byte v of channel c to one of 256 float32
values.  `pixel_table` / `pixel_table_from` make that table, float32 [C][256], ON THE CPU with the operations the loader runs
(ATen's device `div` by a scalar multiplies by a reciprocal: not the same function).  The table is plain data: the stem kernels
apply their own quantizer to it (slfp_conv2d_fwd_u8), so the quantizer's semantics stay in one place.

`expand(x_u8, table)` is the float32 tensor the byte path stands for, x32[n, c, h, w] = table[c][x[n, c, h, w]], made on the device in
one pass (slfp_image_u8_expand_f32): the input of every stem without a byte form, and of training.

fusion.link_image_u8(model, table, example_input) marks the stem of a model; see there.
"""
import torch

from . import _lib

__all__ = ["pixel_table", "pixel_table_from", "expand", "IMAGENET_MEAN", "IMAGENET_STD", "CIFAR_MEAN", "CIFAR_STD"]

# the two constant sets of the reference's loaders (utils/preprocessing.py)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def pixel_table(mean, std):
    """float32 [C][256]: P[c][v] is what ToTensor() + Normalize(mean, std) give byte v in channel c, computed on the CPU with
    torchvision's own operations: uint8 -> float32, div(255), then sub_(mean[c]).div_(std[c]) with float32 mean / std tensors."""
    mean = torch.as_tensor(mean, dtype=torch.float32, device="cpu").reshape(-1)
    std = torch.as_tensor(std, dtype=torch.float32, device="cpu").reshape(-1)
    if mean.numel() != std.numel() or mean.numel() < 1:
        raise ValueError("pixel_table: mean and std must have one entry per channel")
    if bool((std == 0).any()):
        raise ValueError("pixel_table: std evaluated to zero, leading to division by zero")   # as Normalize
    t = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)           # ToTensor
    t = t.repeat(mean.numel(), 1)                                                  # [C][256]
    return t.sub_(mean[:, None]).div_(std[:, None]).contiguous()                   # Normalize


def pixel_table_from(fn, channels):
    """float32 [C][256] of any per-channel elementwise callable: fn gets a uint8 CPU tensor of shape (C, 1, 256) -- a C-channel image
    one pixel high whose row is the ramp 0..255 in every channel -- and returns a tensor of that shape (any float dtype)."""
    ramp = torch.arange(256, dtype=torch.uint8).repeat(int(channels), 1, 1)
    out = fn(ramp)
    if not torch.is_tensor(out) or tuple(out.shape) != (int(channels), 1, 256):
        raise ValueError(f"pixel_table_from: the callable must return a ({int(channels)}, 1, 256) tensor")
    return out.detach().to(device="cpu", dtype=torch.float32).reshape(int(channels), 256).contiguous()


def check_table(table):
    """A pixel table as the library takes it: float32, [C][256], 1 <= C <= 4, contiguous."""
    if not (torch.is_tensor(table) and table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 256
            and 1 <= table.shape[0] <= 4):
        raise ValueError("a pixel table is a float32 tensor of shape (C, 256) with 1 <= C <= 4 (image_u8.pixel_table)")
    return table.contiguous()


def check_pixels(x, table, what="image_u8"):
    """The byte batch a linked stem takes: uint8, logical (N, C, H, W) in channels_last (dense NHWC bytes), on the table's ROCm
    device, C the table's channel count.  Anything else is a TypeError."""
    if not (torch.is_tensor(x) and x.dtype == torch.uint8 and x.dim() == 4):
        raise TypeError(f"{what}: expected a 4-d torch.uint8 pixel batch")
    if not x.is_cuda or x.device != table.device:
        raise TypeError(f"{what}: the pixel batch must live on the weights' ROCm device (got {x.device}, table on {table.device})")
    if x.shape[1] != table.shape[0]:
        raise TypeError(f"{what}: the batch has {x.shape[1]} channels, the pixel table {table.shape[0]}")
    if not x.is_contiguous(memory_format=torch.channels_last):
        raise TypeError(f"{what}: pixel bytes must be channels_last (dense NHWC, as decoded images are); "
                        "NCHW-contiguous bytes are not accepted")


def expand(x, table):
    """x32[n, c, h, w] = table[c][x[n, c, h, w]] as a float32 channels_last tensor, one pass on the device."""
    check_pixels(x, table, "image_u8.expand")
    n, c, h, w = x.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if y.numel():
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().slfp_image_u8_expand_f32(x.data_ptr(), table.data_ptr(), y.data_ptr(), n * h * w, c,
                                                            torch.cuda.current_stream(x.device).cuda_stream))
    return y
