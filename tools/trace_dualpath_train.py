"""One training forward and backward of DualPathRNN at (B, C, T, F) = (2, 64, 11, 13) for every cell and layout of the training side:
SRU dim 3 / 4 / 13 / 14 (13 / 14: the rows layout (B, T, F, 64)), LSTM dim 3 / 4, GRU dim 3 / 4.  Meant to run under a kernel trace, to
compare the launch sequence and the kernel-time sum of two trees (`tools/trace_grids.py --ordered`, `tools/rocpd_stats.py`):

    rocprofv3 --kernel-trace --output-format csv rocpd -d OUT -o t -- python tools/trace_dualpath_train.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import rtfs_net_amd as R

CASES = [("SRU", 3), ("SRU", 4), ("SRU", 13), ("SRU", 14), ("LSTM", 3), ("LSTM", 4), ("GRU", 3), ("GRU", 4)]


def main():
    torch.manual_seed(0)
    for cell, dim in CASES:
        with torch.device("cuda"):  # parameters born on the device: an upload is a runtime copy kernel whose time depends on the host's pages
            mod = R.layers.DualPathRNN(64, 32, dim % 10, kernel_size=8, stride=1, rnn_type=cell, num_layers=4, bidirectional=True).train()
        x = torch.randn(2, 64, 11, 13, device="cuda")
        if dim >= 10:
            x = x.permute(0, 2, 3, 1).contiguous().requires_grad_()
            sru = [p for c in mod.rnn.rnn_lst for p in (c.weight, c.weight_c, c.bias)]
            out = R.layers.dualpath_train(x, dim, mod.norm.gamma, mod.norm.beta, sru, mod.linear.weight, mod.linear.bias)
        else:
            out = mod(x.requires_grad_())
        out.backward(torch.randn_like(out))
        torch.cuda.synchronize()
        assert x.grad is not None and all(p.grad is not None for p in mod.parameters()), (cell, dim)  # no value checks: they would launch kernels
        print(f"{cell} dim {dim}: out {tuple(out.shape)}")


if __name__ == "__main__":
    main()
