"""LinearPolicy -- the policy of Augmented Random Search (Mania, Guy, Recht 2018): y = W x, no bias, no hidden layer.

A build extension (the reference has no linear policy).  theta is W [n_actions, n_inputs] row-major, the parameters()
order of nn.Linear(n_inputs, n_actions, bias=False), and starts at zero as ARS does.  The policy is deterministic:
a discrete env takes the first maximal y_i, a continuous env takes y itself (the env clamps).  forward runs the HIP
kernel (fdr_policy_forward, FDR_POLICY_LINEAR); rollouts run one lane per thread.
"""
import numpy as np
import torch
import torch.nn as nn

from .policy import Policy


class LinearPolicy(Policy):
    KIND = "linear"

    def __init__(self, n_inputs, n_actions, discrete, seed=124, device=None):
        super().__init__(n_inputs, n_actions, seed=seed, device=device)
        self.discrete = bool(discrete)
        self._build_model()
        self._finalize()

    def _init_params(self):
        with torch.no_grad():
            self.model[0].weight.zero_()

    @torch.no_grad()
    def get_action(self, x, deterministic=False):
        y = self.forward(x)
        if self.discrete:
            return int(np.argmax(y[0].cpu().numpy()))   # the first maximal index, as the rollout kernel's scan
        return y.flatten().tolist()

    @torch.no_grad()
    def get_entropy(self, x):
        return 0.0

    @torch.no_grad()
    def get_strategy(self, x):
        return self.forward(np.asarray(x)).cpu().numpy()

    @torch.no_grad()
    def compute_vbn(self, buffer):
        pass

    def _build_model(self):
        self.model = nn.Sequential(nn.Linear(self.input_shape, self.output_shape, bias=False))
