"""CPU restatement of the Silero v5 8 kHz sub-network (test infrastructure; PARITY UNPINNED like oracle/silero.py's 16 kHz graph):

    x[B,288] = 32 context + 256 new samples --reflect-pad right 32--> [B,320]
      --conv1d(basis[130,1,128], stride 64)--> [B,130,4] -> sqrt(re^2+im^2) [B,65,4]
      --Conv1d(65,128,3,s1,p1)+ReLU -> Conv1d(128,64,3,s2,p1)+ReLU -> Conv1d(64,64,3,s2,p1)+ReLU -> Conv1d(64,128,3,s1,p1)+ReLU
      --LSTMCell(128,128) --> ReLU -> Conv1d(128,1,1) -> sigmoid                                             [B,1]

Evaluated in the dtype of the weights given (the tests use float64)."""
import numpy as np
import torch
import torch.nn.functional as F

WINDOW, CONTEXT = 256, 32


def weights64(w):
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in w.items()}


def input_projection(w, x):
    """x [B,288] -> W_ih feat + b_ih + b_hh [B,512] (torch gate order)"""
    xp = F.pad(x.unsqueeze(1), (0, 32), mode="reflect")
    spec = F.conv1d(xp, w["stft_basis"].unsqueeze(1), stride=64)
    re, im = spec[:, :65], spec[:, 65:]
    y = torch.sqrt(re * re + im * im)
    for i, s in enumerate((1, 2, 2, 1)):
        y = F.relu(F.conv1d(y, w[f"enc{i}_w"], w[f"enc{i}_b"], stride=s, padding=1))
    return y.squeeze(-1) @ w["lstm_w_ih"].t() + w["lstm_b_ih"] + w["lstm_b_hh"]


def net_forward(w, x, state):
    gates = input_projection(w, x) + state[0] @ w["lstm_w_hh"].t()
    i_g, f_g, g_g, o_g = gates.chunk(4, dim=1)
    c1 = torch.sigmoid(f_g) * state[1] + torch.sigmoid(i_g) * torch.tanh(g_g)
    h1 = torch.sigmoid(o_g) * torch.tanh(c1)
    return torch.sigmoid(F.relu(h1) @ w["dec_w"].reshape(-1, 1) + w["dec_b"]), torch.stack([h1, c1])


def clip_probs(w, audio, n=None):
    """audio [B,N] -> probs [B, ceil(n/256)] and the final state: zero state and context, last window zero-padded (utils_vad.py:130-146)"""
    x = torch.as_tensor(np.asarray(audio), dtype=torch.float64)
    B, N = x.shape
    n = N if n is None else n
    T = (n + WINDOW - 1) // WINDOW
    xp = torch.zeros((B, CONTEXT + T * WINDOW), dtype=torch.float64)
    xp[:, CONTEXT:CONTEXT + n] = x[:, :n]
    state = torch.zeros((2, B, 128), dtype=torch.float64)
    out = []
    for t in range(T):
        p, state = net_forward(w, xp[:, t * WINDOW:t * WINDOW + CONTEXT + WINDOW], state)
        out.append(p[:, 0])
    return torch.stack(out, 1).numpy(), state.numpy()
