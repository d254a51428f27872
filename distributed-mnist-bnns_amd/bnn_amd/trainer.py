"""The reference's data-parallel BNN training loop (mnist-dist2.py:22-155), on libbnn + RCCL.

    # one process per GPU (torchrun or the reference's mp.spawn style):
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m bnn_amd.trainer --model wide --batch-size 65536 --epochs 1
    python -m bnn_amd.trainer -g 2 --epochs 1          # spawns 2 local ranks itself

Flags keep the reference's names (-n/--nodes, -g/--gpus, -nr/--nr, --epochs, --seed, --lr,
--log-interval; mnist-dist2.py:23-37).  Semantics kept: batch 64 by default (:88), Adam(lr) on
the latent weights (:91; --optimizer sgd: the SGD of the ConvNet scripts, fused as LatentSGD; --optimizer bop:
Bop on the binarized weights, Adam on the rest, fused as LatentBop, with a per-epoch flip-ratio line),
DistributedSampler order with seed 0 and no set_epoch (:100-108),
1-based epochs with the per-batch ``lr *= 0.1`` whenever ``epoch % 40 == 0`` (:126-127), the
.org restore -> step -> clamp protocol (:131-137, here fused into LatentAdam), AverageMeter batch
timing and the reference's log line (:139-146), optional CSVs in the reference's format
(mnist-dist3.py:132-135).  Differences: RCCL instead of gloo, inputs held in HBM
(synthetic MNIST-shaped data unless --idx-images/--idx-labels point at real idx files), fused
BatchNorm+Hardtanh, no fp32 copy of sign(input).  Evaluation (bnn_amd.metrics; all off by default):
--eval-topk K adds the held-out loss, prec@1 and prec@K to --eval N, --eval-idx-images / --eval-idx-labels
evaluate on idx files (t10k), --checkpoint-best PATH keeps the best epoch's weights (utils.save_checkpoint's
is_best), --train-acc appends the training batches' prec@1 to the log line.
"""
import argparse
import os
import time
from datetime import datetime

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from . import functional as BF
from . import nets
from . import nn as BNN
from .checkpoint import load_checkpoint, save_checkpoint
from .graph import GraphedStep
from .data import load_idx_dataset, shard_indices, synthetic_mnist
from .inference import freeze
from .metrics import Meter
from .optim import LatentAdam, LatentBop, LatentSGD
from .parallel import GradExchange

EVAL_SEED = 4321     # --eval's held-out synthetic samples (the training set is seed 1234)


class AverageMeter:
    """utils.py:86-102 semantics (val / sum / count / avg)."""

    def __init__(self):
        self.val = self.avg = self.sum = 0.0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", "--nodes", default=1, type=int)
    ap.add_argument("-g", "--gpus", default=1, type=int, help="processes (GPUs) per node")
    ap.add_argument("-nr", "--nr", default=0, type=int, help="rank of this node")
    ap.add_argument("--epochs", default=10, type=int)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--log-interval", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--model", default="mlp", choices=sorted(nets.MODELS))
    ap.add_argument("--dataset-size", type=int, default=60000, help="synthetic training set size")
    ap.add_argument("--idx-images", default=None)
    ap.add_argument("--idx-labels", default=None)
    ap.add_argument("--graph", action="store_true", help="replay each full batch's step from a HIP graph "
                    "(one process; bnn_amd.graph)")
    ap.add_argument("--fp32-input", action="store_true", help="keep the dataset as fp32 images (u/255) "
                    "instead of u8 pixels")
    ap.add_argument("--max-steps", type=int, default=0, help="stop each epoch after this many steps")
    ap.add_argument("--no-lr-quirk", action="store_true", help="drop the per-batch lr*=0.1 at epoch%%40==0")
    ap.add_argument("--lr-quirk-period", type=int, default=40, help="the 40 of epoch%%40==0 (mnist-dist2.py:126)")
    ap.add_argument("--device-step", action="store_true", help="eager steps on the device step counter (dropout "
                    "seeds and the optimizer as --graph draws them: an eager twin of a --graph run)")
    ap.add_argument("--stochastic", action="store_true", help="stochastic activation binarization in training "
                    "(Binarize(t, 'stoch') on the hidden layers' inputs; eval and --eval stay deterministic)")
    ap.add_argument("--loss", default="ce", choices=("ce", "hinge", "sqhinge"), help="the criterion: ce = "
                    "CrossEntropyLoss on the LogSoftmax output (mnist-dist2.py:118-137); hinge / sqhinge = the mean "
                    "(squared) hinge of models/binarized_modules.py on the logits, one-vs-all +-1 targets")
    ap.add_argument("--optimizer", default="adam", choices=("adam", "sgd", "bop"), help="adam = LatentAdam "
                    "(mnist-dist2.py:91); sgd = LatentSGD, torch.optim.SGD of the reference's ConvNet scripts (mnist.py, mnist-dist.py, "
                    "mnist-mixed.py, mnist-distributed-BNNS2.py), with the flags below; bop = LatentBop, the binary optimizer "
                    "(Helwegen et al. 2019) on the binarized layers' weights and Adam(--lr) on every other parameter")
    ap.add_argument("--momentum", type=float, default=0.0, help="--optimizer sgd")
    ap.add_argument("--dampening", type=float, default=0.0, help="--optimizer sgd")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="--optimizer sgd")
    ap.add_argument("--nesterov", action="store_true", help="--optimizer sgd")
    ap.add_argument("--bop-gamma", type=float, default=1e-4, help="--optimizer bop: the rate of the gradient's moving "
                    "average, in (0, 1]")
    ap.add_argument("--bop-threshold", type=float, default=1e-8, help="--optimizer bop: a weight flips when the average "
                    "exceeds this against it; not negative")
    ap.add_argument("--csv-prefix", default=None, help="write <prefix>_BATCH_TIME.csv / _EPOCH_TIME.csv")
    ap.add_argument("--checkpoint", default=None, help="write a latent-weight checkpoint here after every epoch")
    ap.add_argument("--resume", default=None, help="resume from a checkpoint written by --checkpoint")
    ap.add_argument("--eval", type=int, default=0, metavar="N", help="after every epoch rank 0 freezes the model "
                    "(bnn_amd.inference) and prints its accuracy on N held-out samples")
    ap.add_argument("--eval-topk", type=int, default=0, metavar="K", help="with --eval: also print the held-out loss, "
                    "prec@1 and prec@K (bnn_amd.metrics; utils.accuracy's numbers), K in 1..10")
    ap.add_argument("--eval-idx-images", default=None, help="with --eval N: evaluate on the first N images of this idx "
                    "file (t10k) instead of the synthetic held-out draw; needs --eval-idx-labels")
    ap.add_argument("--eval-idx-labels", default=None)
    ap.add_argument("--checkpoint-best", default=None, metavar="PATH", help="with --eval: write a checkpoint here after "
                    "every evaluation whose prec@1 is above the best so far (utils.save_checkpoint's is_best)")
    ap.add_argument("--train-acc", action="store_true", help="count prec@1 of the training batches on the device and "
                    "append it to the log line")
    ap.add_argument("--backend", default="nccl")
    ap.add_argument("--master-addr", default=os.environ.get("MASTER_ADDR", "127.0.0.1"))
    ap.add_argument("--master-port", default=os.environ.get("MASTER_PORT", "23456"))
    args = ap.parse_args(argv)
    if not 0 <= args.eval_topk <= 10:
        raise SystemExit("--eval-topk K: K must lie in 1..10, the class count (0: off)")
    if (args.eval_idx_images is None) != (args.eval_idx_labels is None):
        raise SystemExit("--eval-idx-images and --eval-idx-labels go together: the held-out set needs both files")
    for flag, on in (("--eval-topk", args.eval_topk > 0), ("--eval-idx-images / --eval-idx-labels",
                     args.eval_idx_images is not None), ("--checkpoint-best", args.checkpoint_best is not None)):
        if on and args.eval <= 0:
            raise SystemExit(f"{flag} needs --eval N: it acts on the evaluation after every epoch")
    return args


def optimizer_kind(state_dict):
    """"adam" / "sgd" / "bop": which optimizer wrote this state_dict, told from its param_groups."""
    groups = state_dict.get("param_groups") or [{}]
    if "gamma" in groups[0]:        # before betas: LatentBop's groups carry Adam's too
        return "bop"
    if "betas" in groups[0]:
        return "adam"
    if "momentum" in groups[0]:
        return "sgd"
    return None


def check_resume_optimizer(path, want, map_location=None):
    """--resume: end with a SystemExit when the checkpoint's optimizer state is the other optimizer's."""
    blob = torch.load(path, map_location=map_location, weights_only=True)
    opt_sd = blob.get("optimizer") if isinstance(blob, dict) else None
    have = optimizer_kind(opt_sd) if opt_sd else None
    if have is not None and have != want:
        raise SystemExit(f"--resume {path}: the checkpoint holds --optimizer {have} state, this run has "
                         f"--optimizer {want}; resume with --optimizer {have}")


def checkpoint_prec1(path, map_location=None):
    """The prec@1 a --checkpoint-best file was written at (its extra["prec1"]), or None."""
    blob = torch.load(path, map_location=map_location, weights_only=True)
    extra = blob.get("extra") if isinstance(blob, dict) else None
    return float(extra["prec1"]) if extra and "prec1" in extra else None


def load_dataset(args, device, rank, as_u8=True):
    """Resident training set: u8 pixels (fc1 applies ToTensor on the bytes) unless the model
    needs the fp32 images (the CNN) or --fp32-input asks for them."""
    if args.idx_images:
        imgs, labels = load_idx_dataset(args.idx_images, args.idx_labels, device)
        return (imgs if as_u8 else imgs.float().div_(255.0)), labels
    # identical synthetic set on every rank (seed 1234); the sampler shards it
    return synthetic_mnist(args.dataset_size, seed=1234, device=device, as_u8=as_u8)


def train(gpu, args):
    world = args.gpus * args.nodes
    rank = args.nr * args.gpus + gpu
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:      # launched by torch.distributed.run
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        gpu = int(os.environ.get("LOCAL_RANK", gpu))
    torch.cuda.set_device(gpu)
    device = torch.device("cuda", gpu)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", args.master_addr)
        os.environ.setdefault("MASTER_PORT", str(args.master_port))
        if args.backend == "nccl":
            from .parallel import init_rccl
            init_rccl(device, rank, world, init_method="env://")
        else:
            dist.init_process_group(args.backend, init_method="env://", world_size=world, rank=rank)
    torch.cuda.manual_seed(args.seed)
    kw = {} if args.loss == "ce" else {"log_softmax": False}      # the hinge criteria take the logits
    model = nets.MODELS[args.model](org_protocol=False, mutate_input=False,
                                    fused_bn=True, stochastic=args.stochastic, **kw).to(device)
    exchange = GradExchange(model) if world > 1 else None
    if args.graph and world > 1:
        raise SystemExit("--graph runs one process (the gradient exchange is not captured)")
    dstep = BF.DeviceStep(device).activate() if (args.graph or args.device_step) else None
    if args.optimizer == "sgd":
        opt = LatentSGD(model.parameters(), lr=args.lr, momentum=args.momentum, dampening=args.dampening,
                        weight_decay=args.weight_decay, nesterov=args.nesterov,
                        clamp_params=nets.binary_params(model), device_step=dstep)
    elif args.optimizer == "bop":
        opt = LatentBop(model.parameters(), lr=args.lr, gamma=args.bop_gamma, threshold=args.bop_threshold,
                        bop_params=nets.binary_weights(model), clamp_params=nets.binary_params(model),
                        device_step=dstep)
        bop_names = {id(p): n for n, p in model.named_parameters()}
    else:
        opt = LatentAdam(model.parameters(), lr=args.lr, clamp_params=nets.binary_params(model), device_step=dstep)
    if args.loss == "ce":
        crit = torch.nn.CrossEntropyLoss()
    else:
        crit = BNN.HingeLoss() if args.loss == "hinge" else BNN.SqrtHingeLoss()     # on the int64 labels
    first_epoch = 1
    if args.resume:
        check_resume_optimizer(args.resume, args.optimizer, map_location="cpu")
        first_epoch = load_checkpoint(args.resume, model, opt, map_location=device) + 1
    best_prec1 = None
    if args.resume and args.checkpoint_best:
        best_prec1 = checkpoint_prec1(args.resume, map_location="cpu")     # carry on from the resumed run's best
    data, targets = load_dataset(args, device, rank, as_u8=args.model != "cnn" and not args.fp32_input)
    idx = torch.tensor(shard_indices(len(data), world, rank), device=device)
    nb = (len(idx) + args.batch_size - 1) // args.batch_size
    T, E = [], []
    graphed = static_x = static_y = None
    frozen = held_x = held_y = ev = None
    is_best = False
    if args.eval > 0 and not isinstance(model, (nets.MLP, nets.BinCNN)):
        raise SystemExit("--eval freezes the binarized MLPs (mlp / small / wide) and the cnn, not --model " + args.model)

    # --train-acc: prec@1 of the training batches, counted on the device from each step's output (one launch,
    # part of a captured step) and read where the loop reads the loss
    train_meter = []

    def _count(out, yb):
        if args.train_acc:
            if not train_meter:
                train_meter.append(Meter(out.shape[1], k=1, device=device))
            train_meter[0].update(out.detach(), yb)
        return out

    def _step(xb, yb):
        for p in model.parameters():
            p.grad = None
        lo = crit(_count(model(xb), yb), yb)
        lo.backward()
        opt.step()
        return lo

    starts = datetime.now()
    for epoch in range(first_epoch, args.epochs + 1):
        T.append(["epoch", epoch])
        start = datetime.now()
        meter = AverageMeter()
        end = time.time()
        model.train()
        for batch_idx in range(nb):
            if args.max_steps and batch_idx >= args.max_steps:
                break
            sel = idx[batch_idx * args.batch_size:(batch_idx + 1) * args.batch_size]
            x, y = data.index_select(0, sel), targets.index_select(0, sel)
            quirk = epoch % args.lr_quirk_period == 0 and not args.no_lr_quirk
            if args.graph and len(sel) == args.batch_size and not quirk:
                # full batches replay one captured step on static buffers (the last, short batch
                # and lr-quirk epochs run eagerly)
                if graphed is None:
                    static_x, static_y = x.clone(), y.clone()
                    loss = None             # drop the last eager step's autograd graph before capturing
                    graphed = GraphedStep(lambda: _step(static_x, static_y), opt, dstep, warmup=1)
                else:
                    static_x.copy_(x)
                    static_y.copy_(y)
                    graphed()
                loss = graphed.out
            else:
                if exchange is not None:
                    exchange.zero_grad()
                else:
                    opt.zero_grad(set_to_none=True)
                loss = crit(_count(model(x), y), y)
                if quirk:
                    opt.param_groups[0]["lr"] *= 0.1
                    graphed = None          # the captured step holds the old lr (Adam's schedule, SGD's argument)
                loss.backward()
                if exchange is not None:
                    exchange.finish()
                opt.step()
            meter.update(time.time() - end)     # host time per batch, as utils.AverageMeter use
            end = time.time()
            if batch_idx % args.log_interval == 0:
                lv = loss.item()                # syncs, like the reference's loss.item()
                if batch_idx * len(x) != 0:
                    T.append([batch_idx * len(x), meter.val])
                acc = ""
                if train_meter:                 # read and reset with the loss: the batches since the last line
                    acc = "\tAcc: {:.2f}".format(train_meter[0].result()["prec1"])
                    train_meter[0].reset()
                if rank == 0:
                    print("Train Epoch: {} [{}/{} ({:.0f}%)]\tLoss: {:.6f} \t Time: {:.3f}({:.3f})".format(
                        epoch, batch_idx * len(x), len(data), 100.0 * batch_idx / nb, lv, meter.val, meter.avg) + acc,
                        flush=True)
        torch.cuda.synchronize()
        if rank == 0:
            print("Training ", epoch, " : " + str(datetime.now() - start), flush=True)
        E.append([datetime.now() - start])
        if args.optimizer == "bop":
            # each binarized layer's flip ratio over the epoch, flips / (numel x steps): one host read
            counts = opt.flip_counts(reset=True)
            if rank == 0:
                print("Flips {} : ".format(epoch) + " ".join(
                    "{} {:.3e}".format(bop_names[id(p)], f / max(1, n * s)) for p, (f, n, s) in counts.items()),
                    flush=True)
        if args.eval > 0 and rank == 0:
            if frozen is None:
                # held-out samples: a draw of bnn_amd.data the training set (seed 1234) does not use
                if args.eval_idx_images:
                    held_x, held_y = load_idx_dataset(args.eval_idx_images, args.eval_idx_labels, device)
                    held_x, held_y = held_x[:args.eval], held_y[:args.eval]     # N clipped to the file's length
                else:
                    held_x, held_y = synthetic_mnist(args.eval, seed=EVAL_SEED, device=device, as_u8=True)
                frozen = freeze(model)
            else:
                frozen.refresh()
            n_eval = len(held_x)
            print("Eval {} : accuracy {:.4f} on {} held-out samples".format(
                epoch, frozen.accuracy(held_x, held_y, batch=max(1, min(n_eval, 65536))), n_eval), flush=True)
            if args.eval_topk > 0 or args.checkpoint_best:
                ev = frozen.evaluate(held_x, held_y, k=max(1, args.eval_topk), batch=max(1, min(n_eval, 65536)))
                if args.eval_topk > 0:
                    print("Eval {} : loss {:.6f} prec@1 {:.2f} prec@{} {:.2f} on {} samples".format(
                        epoch, ev["loss"], ev["prec1"], args.eval_topk, ev["preck"], ev["n"]), flush=True)
                is_best = args.checkpoint_best is not None and (best_prec1 is None or ev["prec1"] > best_prec1)
        if args.checkpoint_best:
            # rank 0 evaluated; every rank joins save_checkpoint (it writes from rank 0 and barriers)
            if world > 1:
                flag = torch.tensor([int(is_best)], device=device)
                dist.broadcast(flag, 0)
                is_best = bool(flag.item())
            if is_best:
                if rank == 0:
                    best_prec1 = ev["prec1"]
                save_checkpoint(args.checkpoint_best, model, opt, epoch,
                                extra={"prec1": best_prec1} if rank == 0 else None)
        if args.checkpoint:
            save_checkpoint(args.checkpoint, model, opt, epoch)
    if rank == 0:
        print("Training complete in: " + str(datetime.now() - starts), flush=True)
        if args.csv_prefix:
            import pandas as pd
            pd.DataFrame(T).to_csv(f"{args.csv_prefix}_BATCH_TIME.csv")
            pd.DataFrame(E).to_csv(f"{args.csv_prefix}_EPOCH_TIME.csv")
    if dstep is not None:
        dstep.deactivate()
    if world > 1:
        dist.destroy_process_group()
    return model


def main(argv=None):
    """Run the trainer; a single-process run returns the trained model."""
    args = parse(argv)
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
        train(int(os.environ.get("LOCAL_RANK", 0)), args)
    elif args.gpus > 1:
        os.environ.setdefault("MASTER_ADDR", args.master_addr)
        os.environ.setdefault("MASTER_PORT", str(args.master_port))
        mp.spawn(train, nprocs=args.gpus, args=(args,))
    else:
        return train(0, args)


if __name__ == "__main__":
    main()
