"""A plain float64 restatement of the DRN stem (test infrastructure, not a test module).

`normalise` is DRN.normalise's arithmetic (models/drn.py:319-321) on the CPU; `stem64` is the two convolutions the fused stem
kernels of csrc/spa_stem.hip compute — layer 0 = relu(conv7x7(3 -> 16) + b0), layer 1 = relu(conv3x3(16 -> 16) + b1) — in
float64 from the operands the kernels receive: w0 (16, 147) in (n, c, ky, kx) order and w1p (16, 144) in (n, ky, kx, c) order
(Engine.drn_stem_d).  With bf16=True the values are rounded where the bf16 kernel documents its rounding: the normalised
input, both weight tensors, layer 0's output before layer 1 reads it, and the output; the biases stay float32."""
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def normalise(x):
    """(B,3,H,W) 0..255 -> float32: x / 255 in float32, then (x - mean) and (x / std) in float64, each rounded to float32."""
    x = torch.as_tensor(x).detach().cpu().float()
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    t = x / 255.0
    t = (t.double() - mean).float()
    return (t.double() / std).float()


def round_bf16(t):
    """float32 value -> the nearest bfloat16 (ties to even), returned as float64."""
    return torch.as_tensor(t).float().to(torch.bfloat16).double()


def stem_weights(w0, w1p):
    """The packed operands as convolution weights: w0 (16,147) -> (16,3,7,7), w1p (16,144) (n,ky,kx,c) -> (16,16,3,3)."""
    w0 = torch.as_tensor(w0).detach().cpu()
    w1p = torch.as_tensor(w1p).detach().cpu()
    return w0.reshape(16, 3, 7, 7), w1p.reshape(16, 3, 3, 16).permute(0, 3, 1, 2)


def stem64(xn, w0, b0, w1p, b1, bf16=False):
    """xn: normalised (B,3,H,W).  Returns (y, y0), both (B,16,H,W) float64: y0 = layer 0's output, y = layer 1's."""
    w0, w1 = stem_weights(w0, w1p)
    b0 = torch.as_tensor(b0).detach().cpu().float().double()
    b1 = torch.as_tensor(b1).detach().cpu().float().double()
    xn = torch.as_tensor(xn).detach().cpu()
    if bf16:
        xn, w0, w1 = round_bf16(xn), round_bf16(w0), round_bf16(w1)
    else:
        xn, w0, w1 = xn.double(), w0.double(), w1.double()
    y0 = torch.relu(F.conv2d(xn, w0, b0, 1, 3))
    if bf16:
        y0 = round_bf16(y0)
    y = torch.relu(F.conv2d(y0, w1, b1, 1, 1))
    if bf16:
        y = round_bf16(y)
    return y, y0
