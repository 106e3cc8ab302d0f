"""What the fused training drivers (``train``, ``train_celeba``, ``train_coco``, ``train_imageonly``, ``train_textonly``,
``train_textonly_multimnist``) share: the meters, the checkpoint file, the KL schedule, the ``--generate`` flags, and the epoch
loops around ONE fused enqueue per batch.  Each driver keeps its own command line, printed lines and checkpoint dict."""
from __future__ import annotations

import os
import shutil

import torch


class AverageMeter(object):
    """multimnist/train.py:26-42"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def save_checkpoint(state, is_best, folder='./', filename='checkpoint.pth.tar'):
    """multimnist/train.py:44-49 (same file names, same dict: see the drivers' ``main``)."""
    os.makedirs(folder, exist_ok=True)
    torch.save(state, os.path.join(folder, filename))
    if is_best:
        shutil.copyfile(os.path.join(folder, filename), os.path.join(folder, 'model_best.pth.tar'))


def kl_schedule():
    """multimnist/train.py:227: the value advances every 5 epochs when --anneal_kl is given."""
    return iter([1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0])


def kl_lambdas(base: float, schedule, epochs: int, anneal_kl: bool = False) -> list:
    """kl_lambda of epochs 1..epochs: ``base`` throughout, or with --anneal_kl the next value of ``schedule`` every 5 epochs, the last
    one kept (multimnist/train.py:226-233 and the scripts modelled on it)."""
    kl, values, out = base, iter(schedule), []
    for epoch in range(1, epochs + 1):
        if anneal_kl and (epoch - 1) % 5 == 0:
            kl = next(values, kl)
        out.append(kl)
    return out


def adam_state_dict(vae, engine, own_only: bool = False) -> dict:
    """The fused engine's flat Adam moments as a ``torch.optim.Adam.state_dict()`` (per-parameter views, cloned), so that
    ``optim.Adam(...).load_state_dict()`` accepts it.  ``own_only``: of the plan's parameters, those that are ``vae``'s own (a
    uni-modal model lives on half of a multimodal plan)."""
    st = engine.state
    step = int(engine.adam_state[0].item())
    own = None
    if own_only:
        plan_name = getattr(vae, "plan_name", lambda n: vae._core.prefix + n)      # (mnist.VAE's keys have no .net. level)
        own = {plan_name(n) for n, _ in vae.named_parameters()}
    state = {}
    for name, shape, off in st.table:
        if own is not None and name not in own:
            continue
        numel = 1
        for s in shape:
            numel *= s
        state[len(state)] = {'step': torch.tensor(float(step)),
                             'exp_avg': engine.exp_avg[off:off + numel].view(shape).clone(),
                             'exp_avg_sq': engine.exp_avg_sq[off:off + numel].view(shape).clone()}
    group = {'lr': engine.lr, 'betas': tuple(engine.betas), 'eps': engine.eps, 'weight_decay': 0, 'amsgrad': False,
             'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
             'decoupled_weight_decay': False, 'params': list(range(len(state)))}
    return {'state': state, 'param_groups': [group]}


def add_generate_flags(parser, generate_help: str) -> None:
    """``--generate`` and what goes with it: fresh MultiMNIST canvases made on the device (multimnist_gen.MultiMNISTStream)."""
    parser.add_argument('--generate', action='store_true', default=False, help=generate_help)
    parser.add_argument('--mnist_train', type=str, default='', help='--generate: MNIST training split, a .pt file holding (uint8 (N,28,28), int64 (N,))')
    parser.add_argument('--mnist_test', type=str, default='', help='--generate: MNIST test split, same layout')
    parser.add_argument('--epoch_size', type=int, default=60000, metavar='N', help='--generate: canvases per training epoch (default: 60000)')
    parser.add_argument('--min_digits', type=int, default=0, help='--generate: minimum number of digits per canvas (datasets.py: 0)')
    parser.add_argument('--max_digits', type=int, default=2, help='--generate: maximum number of digits per canvas (datasets.py: 2; at most 4)')


def mnist_digit_sources(args):
    """(training digits, test digits) of a ``--generate`` run, each (uint8 (N,28,28), int64 (N,)): synthetic, or the two files."""
    if args.synthetic > 0:
        from . import data as D
        return D.synthetic_mnist(args.synthetic, seed=args.seed), D.synthetic_mnist(args.synthetic, seed=args.seed + 1)
    if args.mnist_train and args.mnist_test:
        from .make_multimnist import load_mnist_pt
        return load_mnist_pt(args.mnist_train), load_mnist_pt(args.mnist_test)
    raise SystemExit("--generate needs --mnist_train FILE.pt and --mnist_test FILE.pt, or --synthetic N for synthetic digits")


def train_epoch(loader, step, batch_size: int, log_interval: int, line, n_total: int, n_losses: int = 1, log=print) -> tuple:
    """One training epoch.  ``step(batch)`` enqueues the fused step and returns its ``n_losses`` losses as a device tensor; nothing is
    synchronised but for ONE read-back per ``log_interval`` batches (the reference synchronises per batch), which feeds the meters
    and is followed by ``log(line(samples seen, n_total, percent of the epoch, meter averages))``.  Returns the meter averages."""
    meters = tuple(AverageMeter() for _ in range(n_losses))
    pending = []

    def drain():
        for row in torch.stack(pending).cpu().tolist():
            for m, v in zip(meters, row):
                m.update(v, batch_size)
        pending.clear()

    for batch_idx, batch in enumerate(loader):
        pending.append(step(batch).reshape(n_losses).clone())       # device tensor, no sync
        if batch_idx % log_interval == 0:
            drain()
            log(line(batch_idx * batch_size, n_total, 100. * batch_idx / max(len(loader), 1), tuple(m.avg for m in meters)))
    if pending:
        drain()
    return tuple(m.avg for m in meters)


def eval_epoch(loader, evaluate, n_losses: int, device, reduce=None) -> list:
    """One test epoch: ``evaluate(batch)`` returns ``n_losses`` losses as a device tensor; they are summed on the device, divided by
    the number of batches, handed to ``reduce`` (data parallel: the ranks' average) and read back once."""
    acc = torch.zeros(n_losses, device=device)
    nb = 0
    for batch in loader:
        acc += evaluate(batch).reshape(n_losses)
        nb += 1
    acc = acc / max(nb, 1)
    if reduce is not None:
        acc = reduce(acc)
    return acc.cpu().tolist()
