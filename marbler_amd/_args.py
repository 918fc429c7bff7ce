"""What every Python launch wrapper says about its arguments, stated once: what a tensor argument must be, how many rows an
episode takes in a strided batch, which stream a launch goes on, and how a return code becomes an exception.  Host code only:
nothing here touches a device or needs the library."""
import ctypes as C

import torch

from ._lib import RobogymError

VALUE = (ValueError, ValueError)        # check_tensor(errors=): a caller whose every refusal is a ValueError


def _wanted(name, dtypes, shape, contiguous, got):
    """check_tensor's one wording: what `name` must be, and what was given instead."""
    kinds = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    what, of = (f"a contiguous {kinds} tensor", " of shape ") if contiguous else (f"a tensor of dtype {kinds}", " and shape ")
    return f"{name} must be {what}{'' if shape is None else of + str(tuple(shape))}, got {got}"


def check_tensor(name, t, dtypes, shape, device=None, contiguous=True, errors=(TypeError, ValueError)):
    """`t` must be a tensor of one of `dtypes` and of `shape` (None: any), on `device` (None: anywhere), contiguous if asked.
    errors: the classes raised for (not a tensor, a wrong dtype); everything else is a ValueError.  Returns t."""
    if not isinstance(t, torch.Tensor):
        raise errors[0](_wanted(name, dtypes, shape, contiguous, type(t).__name__))
    if t.dtype not in dtypes:
        raise errors[1](_wanted(name, dtypes, shape, contiguous, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(_wanted(name, dtypes, shape, contiguous, f"the shape {tuple(t.shape)}"))
    if contiguous and not t.is_contiguous():
        raise ValueError(_wanted(name, dtypes, shape, contiguous, f"the strides {t.stride()}"))
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, not on {device}")
    return t


def episode_pitch(name, t, inner):
    """The rows an episode takes in `t` ([B, rows, *inner] with the last dimensions contiguous), from its batch stride."""
    want, row = [], 1
    for d in reversed(inner):
        want.insert(0, row)
        row *= d
    want.insert(0, row)
    # (a dimension of size 1 has no stride to speak of)
    if any(t.shape[1 + k] > 1 and t.stride(1 + k) != want[k] for k in range(len(want))):
        raise ValueError(f"{name}: the last {len(want)} dimensions must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
    B, rows = t.shape[0], t.shape[1]
    if B == 1:
        return rows
    if t.stride(0) % row != 0 or t.stride(0) < rows * row:
        raise ValueError(f"{name}: the batch stride {t.stride(0)} must be a multiple of {row} and at least {rows * row}")
    return t.stride(0) // row


def shared_pitch(prefix, tensors, rows):
    """tensors: (name, [B, rows, *inner] tensor or None, inner) of arrays a launch addresses with ONE pitch -> that pitch;
    `rows` when every one of them is None (the wrapper then allocates them dense)."""
    pitch = None
    for name, t, inner in tensors:
        if t is None:
            continue
        p = episode_pitch(prefix + name, t, inner)
        if pitch not in (None, p):
            raise ValueError(f"{prefix}{', '.join(n for n, _, _ in tensors)} must take the same number of rows per episode ({pitch}, {p})")
        pitch = p
    return rows if pitch is None else pitch


def launch_stream(stream, device):
    """The torch stream a launch goes on (None: the device's current one) and its raw handle for the C ABI."""
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return stream, C.c_void_p(stream.cuda_stream)


def launch_error(rc, text, refuses=True):
    """The exception for a handle-free entry's nonzero `rc` and last-error text: RobogymError for a launch that failed,
    ValueError for arguments the entry refuses (refuses=False: the wrapper has checked them all, every code is a failure)."""
    return (RobogymError if rc == -30 or not refuses else ValueError)(f"({rc}) {text}")
