"""`model-update-bn` driver: re-estimate the running statistics (`mean` / `stdinv`) of every batch norm of a model from
test-mode activations, leaving every other parameter as it is. Mirrors denet/model/update_bn.py of the reference:

  1. the layers (:44-51): top-level `batchnorm` / `batchnorm-relu` layers and those among the `layers` of each `resnet`, in
     model order, each resnet's in its stored order; batch norms nested anywhere else are not touched (they are logged), nor
     are disabled ones (they have no statistics) or layers in group mode (normGroups > 0: per-sample statistics, nothing stored;
     they are logged as skipped, and a model with no other batch norm is written back unchanged);
  2. sequential (:53-60): layer i is estimated from test-mode forward passes in which every batch norm in front of it
     normalises with its stored statistics, those of the layers < i already being the new ones; the pass records the
     per-channel mean and biased variance of the RAW input of layer i;
  3. the per-batch means and variances are averaged (not pooled) in float64 over the n = size // batch_size full batches,
     the padded last batch is never used;
  4. mean = f32(sum_mean / n), stdinv = 1 / sqrt(f32(sum_var / n) + 1e-5) in float32 (:62-66); eps is the literal 1e-5.

The moments are taken on the device (csrc/bn_moments.hip) inside the batch norm's own test-mode forward (BatchNormLayer.forward,
`bn_probe`), with no host round trip per batch. The sweep of layer i runs with the batch norm fold of inference switched off
(ops.infer_fold: a folded batch norm never runs its own forward and its input holds normalised values - the reference has no
fold), and ends after the top-level layer that holds layer i (ModelCNN.forward `stop_after`). Writing the statistics bumps
ops.WEIGHTS_VERSION, so the next sweep and any later inference rebuild what they derive from them.

The reference script calls `data.prepare(...)` (:40), which its own dataset module does not have. The data path here is that
of model-predict: dataset.load(input, extension, is_training=True) + shuffle() + load_from_subset(0) + export(batch_size).
`--seed` (an addition) seeds `random` / `numpy.random` before the shuffle; without it the behaviour is the reference's.
With fewer samples than one batch (n == 0) the tool raises and writes nothing (the reference would write NaN).
"""
import argparse
import random
import sys

import numpy

from . import model_cnn
from .model_cnn import walk_layers

BN_TYPES = ("batchnorm", "batchnorm-relu")
DEVICE_BUDGET = 16 << 30       # bytes of batches kept on the device across all sweeps


def _select(model):
    """[(batch norm, top-level layer holding it)] in the reference's order, and the batch norms left out"""
    chosen = []
    for layer in model.layers:
        if layer.type_name in BN_TYPES:
            chosen.append((layer, layer))
        elif layer.type_name == "resnet":
            chosen += [(l, layer) for l in layer.layers if l.type_name in BN_TYPES]
    # (a group-mode layer - normGroups > 0, DESIGN.md section 21 - has no running statistics to estimate: left out, and logged)
    chosen = [(l, top) for l, top in chosen if l.enabled and not l.norm_groups]
    ids = set(id(l) for l, _ in chosen)
    skipped = [l for l in walk_layers(model.layers) if l.type_name in BN_TYPES and id(l) not in ids]
    return chosen, skipped


def select_bn_layers(model):
    """the enabled batch norms update_bn estimates, in order (update_bn.py:44-51)"""
    return [l for l, _ in _select(model)[0]]


def update_bn(model, batches, log=None, device_budget=DEVICE_BUDGET):
    """re-estimates the statistics of select_bn_layers(model) from `batches` (full batches only: (B, C, H, W) float32 arrays or
    device tensors). Returns [(layer, old_mean, new_mean, old_stdinv, new_stdinv)]."""
    import torch
    from .. import ops
    log = log or (lambda *a: None)
    n = len(batches)
    if n == 0:
        raise ValueError("update_bn: no full batch of %i samples" % model.batch_size)
    chosen, skipped = _select(model)
    log("Found %i batch norm layers" % len(chosen))
    for l in skipped:
        log("Skipping batch norm layer %i (%s)" % (l.layer_index, "disabled" if not l.enabled else
                                                    "group norm, %d groups: no running statistics" % l.norm_groups if l.norm_groups
                                                    else "not top-level or in a resnet"))
    if not chosen:
        log("No batch norm layer with running statistics: nothing to estimate, the model is left unchanged")
        return []
    if not model._packed:
        model.pack_device()
    nbytes = sum(int(numpy.prod(b.shape)) * 4 for b in batches)
    if nbytes <= device_budget:
        # uploaded once, read by every sweep (ModelCNN._upload_input reads a device batch in place)
        batches = [b.cuda().float().contiguous() if isinstance(b, torch.Tensor)
                   else torch.from_numpy(numpy.ascontiguousarray(b, dtype=numpy.float32)).cuda() for b in batches]
    out = []
    # (the statistics are those of the exact fp32 passes whatever ops.INFER_PRECISION / DENET_INFER_BF16 say)
    with ops.infer_fold(False), ops.infer_precision("fp32"):
        for i, (layer, top) in enumerate(chosen):
            log("Estimating mean and var for layer %i with %i batches" % (i, n))
            shape = layer.input_shape
            C = shape[1]
            ws = ops.bn_moments_workspace(int(numpy.prod(shape)) // C, C)
            acc = torch.zeros(2, C, dtype=torch.float64, device="cuda")
            old_mean, old_stdinv = layer.mean.get_value().copy(), layer.stdinv.get_value().copy()
            for b in batches:
                model.forward(b, None, train=False, stop_after=top, bn_probe=(layer, acc, ws))
            ops.bn_moments_finish(acc, n, layer.mean.dev, layer.stdinv.dev, eps=1e-5)
            # get_value() refreshes the host copies (export_json, a later pack_device) from the device
            out.append((layer, old_mean, layer.mean.get_value().copy(), old_stdinv, layer.stdinv.get_value().copy()))
    return out


def build_parser():
    parser = argparse.ArgumentParser(description="Re-estimate the batch norm statistics of a model")
    from ..common import logging
    logging.add_arguments(parser)
    parser.add_argument("--model", required=True, help="input model file")
    parser.add_argument("--output", required=True, help="output model file")
    parser.add_argument("--input", required=True, help="The folder with data")
    parser.add_argument("--extension", default="png", help="Image file extension")
    parser.add_argument("--batch-size", type=int, default=128, help="Size of processing batchs")
    parser.add_argument("--thread-num", default=4, type=int, help="Number of threads for dataset loading")
    parser.add_argument("--seed", default=None, type=int, help="seed of random / numpy.random before the shuffle (default: unseeded)")
    return parser


def load_batches(input, extension, batch_size, thread_num=1, seed=None):
    """the full batches of the shuffled first subset, as model-update-bn reads them: [(batch_size, C, H, W) float32 arrays]"""
    from .. import dataset
    if seed is not None:
        random.seed(seed)
        numpy.random.seed(seed)
    data = dataset.load(input, extension, is_training=True, thread_num=thread_num)
    data.shuffle()
    data.load_from_subset(0)
    if len(data.data) // batch_size == 0:
        return []
    dataset_x, _, dataset_size = data.export(batch_size)
    return [dataset_x[b * batch_size:(b + 1) * batch_size] for b in range(dataset_size // batch_size)]


def main(argv=None):
    args = build_parser().parse_args(argv)
    from ..common import logging
    logging.init(args)
    logging.info("Loading model: ", args.model)
    model = model_cnn.load_from_file(args.model, args.batch_size)
    logging.info("Class labels:\n", model.class_labels)
    logging.info("Loading Dataset...")
    batches = load_batches(args.input, args.extension, args.batch_size, args.thread_num, args.seed)
    if not batches:
        raise ValueError("model-update-bn: fewer samples in %s than one batch of %i; %s is not written"
                         % (args.input, args.batch_size, args.output))
    for i, (_, old_mean, new_mean, old_stdinv, new_stdinv) in enumerate(update_bn(model, batches, log=logging.info)):
        logging.verbose("Layer %i - Old Mean:" % i, old_mean)
        logging.verbose("Layer %i - New Mean:" % i, new_mean)
        logging.verbose("Layer %i - Old Std:" % i, old_stdinv)
        logging.verbose("Layer %i - New Std:" % i, new_stdinv)
    model_cnn.save_to_file(model, args.output)
    logging.info("Done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
