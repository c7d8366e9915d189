"""Training step / epoch of the caption task and the data-parallel gradient exchange.

Restates reference train.py:113-148 (train_epoch), train.py:20-49 (optimizer / scheduler factory)
and replaces torch.nn.parallel.DistributedDataParallel (train.py:217-219) with an explicit bucketed
all-reduce of the flat gradient buffer over RCCL (torch.distributed 'nccl' on ROCm), launched per
bucket as soon as the backward schedule has enqueued the kernels that complete it, so the exchange
of the generator gradients (a third of the bytes, ready first) overlaps the rest of backward."""
from .exchange import GradExchange, ShardedExchange
from .optim import FusedAdam, build_optimizer
from .step import CaptionTrainer, scst_epoch, train_epoch
