"""Model surgery — the operations of denet/model/modify.py (:37-193) that assemble a DeNet detector from a
classifier: --class-num, --image-size, --use-cudnn-pool (:62-68), --convert-bn-relu (:76-113), --modify-bn (:115-131), --layer-remove
(:153-156), --layer-insert N:DESC (:161-175), --layer-append (:177-184). Like the reference every edit goes
through the JSON form and a reload, so shapes and wiring are rebuilt from scratch. --modify-bn-renorm R D IT is this build's
own: the switch for the batch renormalisation the reference carries parameters for and keeps commented out (batch_norm.py:65-73).
So is --modify-bn-groups G: the same traversal sets the key normGroups, which runs the batch norms as group norms (DESIGN.md
section 21)."""
import copy

from . import model_cnn


def _reload(model, json_obj=None):
    json_obj = model.export_json() if json_obj is None else json_obj
    new = model_cnn.load_from_json(json_obj, model.batch_size)
    new.class_labels = model.class_labels
    return new


def set_class_num(model, class_num):
    j = model.export_json()
    j["classNum"] = class_num
    return _reload(model, j)


def set_image_size(model, width, height):
    j = model.export_json()
    j["dataShape"] = (3, height, width)
    return _reload(model, j)


def use_cudnn_pool(model):
    """modify.py:62-68: every pool layer with ignore_border false gets pad (1, 1) and ignore_border true, whatever its window is
    (the published ResNet base models carry one, a 3x3 stride-2 stem pool); a model without such a layer is returned as it is"""
    j = model.export_json()
    changed = False
    for l in j["layers"]:
        if l["type"] == "pool" and not l["ignoreBorder"]:
            l["pad"] = (1, 1)
            l["ignoreBorder"] = True
            changed = True
    return _reload(model, j) if changed else model


def _bn_to_bnrelu(bn_json):
    out = {"type": "batchnorm-relu", "layers": []}
    for k in ("momentum", "eps", "mean", "std", "gamma", "bias"):
        out[k] = bn_json[k]
    if bn_json.get("renormMaxR", 1.0) > 1.0 or bn_json.get("renormMaxD", 0.0) > 0.0:
        for k in RENORM_KEYS:          # a renorm-active layer stays one (the fused layer writes the keys only then)
            if k in bn_json:
                out[k] = bn_json[k]
    if bn_json.get("normGroups", 0):
        out["normGroups"] = bn_json["normGroups"]      # a group-mode layer stays one
    return out


RENORM_KEYS = ("renormMaxR", "renormMaxD", "renormMaxIt")


def modify_bn_renorm(model, max_r, max_d, max_it):
    """--modify-bn-renorm R D IT: the batch-renormalisation limits (the reference's commented-out block, denet/layer/batch_norm.py:
    65-73) of every batchnorm and batchnorm-relu layer and of the bnParam of every residual block; modify_bn's traversal.
    R = 1, D = 0 switches it off again: the keys leave every place that does not carry them by default. A top-level `batchnorm`
    always exports the three keys, so it gets the values as given: after `1 0 0` its renormMaxIt reads 0 (the grammar's default),
    also where the file carried the constructor's 10 before, as older and reference files do - the value has no effect on a
    layer that is switched off"""
    from ..layer.batch_norm import renorm_active, renorm_check
    renorm_check(max_r, max_d, max_it)
    max_r, max_d, max_it = float(max_r), float(max_d), int(max_it) if float(max_it).is_integer() else float(max_it)
    upd = {"renormMaxR": max_r, "renormMaxD": max_d, "renormMaxIt": max_it}
    active = renorm_active(max_r, max_d)

    def edit(d, always):
        if active or always:
            d.update(upd)
        else:
            for k in RENORM_KEYS:
                d.pop(k, None)

    j = model.export_json()
    for l in j["layers"]:
        if l["type"] in ("batchnorm", "batchnorm-relu"):
            edit(l, l["type"] == "batchnorm")
        elif l["type"] == "resnet":
            l["bnParam"] = dict(l.get("bnParam", {}))
            edit(l["bnParam"], False)
            for s in l["layers"]:
                if s["type"] in ("batchnorm", "batchnorm-relu"):
                    edit(s, False)
    return _reload(model, j)


def modify_bn_groups(model, groups):
    """--modify-bn-groups G: group normalisation for every batchnorm and batchnorm-relu layer and the bnParam
    of every residual block, where it reaches every norm of the block; modify_bn_renorm's traversal. 0 goes back to batch
    statistics: the key leaves every place (it is written only when it is not 0). Refuses, naming the layer, when G does not
    divide a layer's channel count"""
    from ..layer.batch_norm import BatchNormLayer, norm_groups_check
    groups = norm_groups_check(groups, what="--modify-bn-groups")
    if groups:
        for l in model_cnn.walk_layers(model.layers):
            if isinstance(l, BatchNormLayer) and l.enabled and l.input_shape[1] % groups:
                raise ValueError("--modify-bn-groups %d: layer %d (%s%s) has %d channels, which %d does not divide"
                                 % (groups, l.layer_index, l.type_name, "" if l in model.layers else ", inside a residual block",
                                    l.input_shape[1], groups))

    def edit(d):
        if groups:
            d["normGroups"] = groups
        else:
            d.pop("normGroups", None)

    j = model.export_json()
    for l in j["layers"]:
        if l["type"] in ("batchnorm", "batchnorm-relu"):
            if l.get("enabled", True):
                edit(l)
        elif l["type"] == "resnet":
            l["bnParam"] = dict(l.get("bnParam", {}))
            if l["bnParam"].get("enabled", True):
                edit(l["bnParam"])
            for s in l["layers"]:
                if s["type"] in ("batchnorm", "batchnorm-relu") and s.get("enabled", True):
                    edit(s)
    return _reload(model, j)


def convert_bn_relu(model):
    """fuse [batchnorm, activation(relu)] pairs, at top level and inside `original` residual blocks"""
    j = model.export_json()
    src = j["layers"]
    dst = []
    i = 0
    while i < len(src):
        l = src[i]
        nxt = src[i + 1] if i + 1 < len(src) else None
        if l["type"] == "batchnorm" and nxt is not None and nxt["type"] == "activation" and nxt["activation"] == "relu" \
                and i + 1 < len(src) - 0:
            dst.append(_bn_to_bnrelu(l))
            i += 2
            continue
        if l["type"] == "resnet" and "bnrelu" not in l["version"] and l["activation"] == "relu":
            # the reference rewrites sub-layers [2],[3] (and [4],[5] with a bottleneck) of `original` blocks
            # (modify.py:91-106); fusing every [batchnorm, activation] pair of the block is the same edit for
            # those and also covers pre-activation blocks (which the reference's index arithmetic does not)
            l = copy.copy(l)
            subs, fused, k = list(l["layers"]), [], 0
            while k < len(subs):
                nx = subs[k + 1] if k + 1 < len(subs) else None
                if subs[k]["type"] == "batchnorm" and nx is not None and nx["type"] == "activation" \
                        and nx["activation"] == "relu":
                    fused.append(_bn_to_bnrelu(subs[k]))
                    k += 2
                else:
                    fused.append(subs[k])
                    k += 1
            l["layers"] = fused
            l["version"] = l["version"] + ",bnrelu"
        dst.append(l)
        i += 1
    j["layers"] = dst
    return _reload(model, j)


def modify_bn(model, enabled, momentum, eps):
    j = model.export_json()
    upd = {"enabled": bool(enabled), "momentum": float(momentum), "eps": float(eps)}
    for l in j["layers"]:
        if l["type"] == "batchnorm":
            l.update(upd)
        elif l["type"] == "resnet":
            l["bnParam"] = dict(l.get("bnParam", {}), **upd)
            for s in l["layers"]:
                if s["type"] in ("batchnorm", "batchnorm-relu"):
                    s["momentum"], s["eps"] = upd["momentum"], upd["eps"]
    return _reload(model, j)


def layer_remove(model, n):
    if n <= 0:
        return model
    j = model.export_json()
    j["layers"] = j["layers"][:-n]
    return _reload(model, j)


def layer_insert(model, inserts, activation="relu", border_mode="half", weight_init="he-backward"):
    """inserts: ["N:DESC", ...]; N indexes the CURRENT layer list including the initial layer (modify.py:163-172)"""
    for s in inserts:
        index, desc = s.split(":")
        index = int(index)
        if index > len(model.layers):
            raise Exception("Error: index %i too large (%i layers)" % (index, len(model.layers)))
        before = list(model.layers[:index])
        after = list(model.layers[index:])
        n0 = len(before)
        model.build_layer(desc, before, activation, border_mode, weight_init)
        new_json = [l.export_json() for l in before[n0:]]
        j = model.export_json()
        j["layers"] = j["layers"][:index - 1] + new_json + j["layers"][index - 1:]
        model = _reload(model, j)
    return model


def layer_append(model, descs, activation="relu", border_mode="half", weight_init="he-backward"):
    if isinstance(descs, str):
        descs = descs.split()
    for desc in descs:
        model.build_layer(desc, model.layers, activation, border_mode, weight_init)
    model._packed = False
    return _reload(model)


def merge_splits(model):
    """--merge (modify.py:53-60): split points become plain pass-throughs (they already execute as such here)"""
    j = model.export_json()
    for l in j["layers"]:
        if l["type"] == "split":
            l["enabled"] = False
        elif l["type"] == "skip-src":
            l["split"] = False
    return _reload(model, j)


def set_activation(model, activation):
    """modify.py:48-51: every activation / residual layer takes the activation named on the command line"""
    from ..layer.activation import check_activation
    check_activation(activation)
    j = model.export_json()
    changed = False
    for index, l in enumerate(j["layers"]):
        if l["type"] == "resnet" and "bnrelu" in l["version"] and activation != "relu" and l.get("activation") != activation:
            # a block converted by --convert-bn-relu stores `batchnorm-relu` sub-layers; with any other activation the block is
            # built from `batchnorm` + `activation` sub-layers and the stored ones no longer line up (the reference dies on the
            # same mismatch when it reloads)
            raise ValueError("--activation %s: layer %i is a residual block converted by --convert-bn-relu (version '%s', fused "
                             "batchnorm-relu sub-layers), which only 'relu' can run; set the activation before converting"
                             % (activation, index + 1, l["version"]))
        if l["type"] in ("activation", "resnet") and l.get("activation") != activation:
            l["activation"] = activation
            changed = True
    return _reload(model, j) if changed else model


def modify_layer(model, layer_name, assignments):
    """--modify-layer TYPE key=value ...: set attributes of the FIRST layer of that type (modify.py:130-146); the value
    takes the type of the attribute it replaces. The edit goes through the layer's JSON keys and a reload."""
    for index, layer in enumerate(model.layers):
        if layer.type_name != layer_name:
            continue
        before = layer.export_json()
        for a in assignments:
            name, text = a.split("=")
            old = getattr(layer, name)
            if type(old) is bool:
                value = {"True": True, "False": False, "0": False, "1": True}[text]
            elif type(old) is tuple:
                # a pair-typed attribute (stride, dilation): `dilation=2` -> (2, 2), `dilation=2,3` -> (2, 3)
                from .. import common
                parts = tuple(common.convert_num(t) for t in text.split(","))
                value = parts * len(old) if len(parts) == 1 else parts
            else:
                value = type(old)(text)
            setattr(layer, name, value)
        after = layer.export_json()
        if after == before:
            raise Exception("--modify-layer: none of %s is part of the exported state of '%s'" % (assignments, layer_name))
        j = model.export_json()
        j["layers"][index - 1] = after
        return _reload(model, j)
    raise Exception("--modify-layer: no layer of type '%s'" % layer_name)


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Modify a model file (same flags as the reference's model-modify)")
    from ..common import logging
    logging.add_arguments(parser)
    parser.add_argument("--seed", type=int, default=23455, help="Random Seed for weights")
    parser.add_argument("--input", type=str, required=True)
    parser.add_argument("--output", type=str, required=True)
    parser.add_argument("--class-num", type=int, default=None)
    parser.add_argument("--image-size", nargs="+", type=int, default=None)
    parser.add_argument("--use-cudnn-pool", default=False, action="store_true",
                        help="every border-keeping pool layer (ignoreBorder false, `P.B`) becomes a cuDNN-mode one: pad (1, 1), "
                             "ignoreBorder true")
    parser.add_argument("--convert-bn-relu", default=False, action="store_true")
    parser.add_argument("--merge", default=False, action="store_true", help="merge split layers")
    parser.add_argument("--modify-bn", default=None, nargs="+", type=str, help="enabled momentum eps for batch norm")
    parser.add_argument("--modify-bn-renorm", default=None, nargs=3, type=float, metavar=("R", "D", "IT"),
                        help="batch renormalisation for every batch norm (training only): r is clipped to [1/R, R], d to [-D, D], the "
                             "limits open over the first IT epochs (0: open from the start); 1 0 0 switches it off (a top-level batchnorm "
                             "layer then carries renormMaxIt 0, whatever it carried before)")
    parser.add_argument("--modify-bn-groups", default=None, type=int, metavar="G",
                        help="group normalisation for every batch norm (training and inference): statistics per sample over G groups "
                             "of consecutive channels; G must divide every layer's channel count; 0 goes back to batch statistics")
    parser.add_argument("--modify-layer", default=None, nargs="+", type=str, help="TYPE key=value ...")
    parser.add_argument("--layer-insert", default=[], nargs="+", help="insert layer at position N:DESC")
    parser.add_argument("--layer-remove", default=0, type=int, help="remove N layer from end")
    parser.add_argument("--layer-append", default=[], nargs="+", type=str, help="append layers to end")
    parser.add_argument("--border-mode", default="half")
    parser.add_argument("--activation", default="relu")
    parser.add_argument("--weight-init", nargs="+", default=["he-backward"])
    return parser


def main(argv=None):
    """the edits of the reference's model-modify (modify.py:37-193)"""
    import random
    import numpy
    args = build_parser().parse_args(argv)
    random.seed(args.seed)
    numpy.random.seed(args.seed)
    model = model_cnn.load_from_file(args.input)
    # the reference edits the loaded object and reloads ONCE (modify.py:153-159); here every edit reloads, so the ones
    # that drop layers run before the ones that change the input geometry (and --use-cudnn-pool first of all: a border-keeping
    # pool that the new geometry would refuse is already a cuDNN-mode one by then)
    if args.use_cudnn_pool:
        model = use_cudnn_pool(model)
    if args.modify_bn is not None:
        model = modify_bn(model, bool(args.modify_bn[0]), float(args.modify_bn[1]), float(args.modify_bn[2]))
    if args.modify_bn_renorm is not None:
        model = modify_bn_renorm(model, *args.modify_bn_renorm)
    if args.modify_bn_groups is not None:
        model = modify_bn_groups(model, args.modify_bn_groups)
    if args.convert_bn_relu:
        model = convert_bn_relu(model)
    model = layer_remove(model, args.layer_remove)
    if args.class_num is not None:
        model = set_class_num(model, args.class_num)
    if args.image_size is not None:
        model = set_image_size(model, args.image_size[0], args.image_size[1])
    model = set_activation(model, args.activation)
    if args.merge:
        model = merge_splits(model)
    if args.modify_layer is not None:
        model = modify_layer(model, args.modify_layer[0], args.modify_layer[1:])
    if len(args.layer_insert) > 0:
        model = layer_insert(model, args.layer_insert, args.activation, args.border_mode, args.weight_init)
    if len(args.layer_append) > 0:
        model = layer_append(model, args.layer_append, args.activation, args.border_mode, args.weight_init)
    model_cnn.save_to_file(model, args.output)
    for layer in model.layers:
        print(layer)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
