#!/bin/bash
# The getting-started classifier on CIFAR-10 with this build's model-train: a nine-layer network with batch norm, dropout,
# `same` 2x2 / 1x1 convolutions behind every 3x3 one and an `R.C[6]` head (a 6x6 convolution to a 4x4 map, classified at
# its centre pixel), 90 epochs of SGD at batch 32 on one GPU.
#   examples/simple-cifar10.sh <train dir> <test dir>
# Both directories hold one sub-folder of PNG images per class. Output goes to ./simple-cifar10-model (EPOCHS=N to shorten).
set -e
TRAIN_DIR=${1:?training directory (one folder of PNGs per class)}
TEST_DIR=${2:?test directory (one folder of PNGs per class)}
DIR="$( cd "$( dirname "${BASH_SOURCE[0]}" )" && pwd )/.."
BIN=$DIR/bin
EPOCHS=${EPOCHS:-90}
TRAIN_DIR=$(cd "$TRAIN_DIR" && pwd)
TEST_DIR=$(cd "$TEST_DIR" && pwd)

MODEL_DESC=$(PYTHONPATH=$DIR python -c "from denet_amd.model import zoo; print(zoo.SIMPLE_CIFAR10_DESC)")
OUTPUT_DIR=./simple-cifar10-model
mkdir -p $OUTPUT_DIR && cd $OUTPUT_DIR
echo "training $MODEL_DESC"
echo "  train $TRAIN_DIR, test $TEST_DIR, logs in $PWD/train.out / train.err"

# --distort-mode is accepted and unused, as in the reference's own driver
$BIN/model-train --seed 0 --distort-mode o4 --solver sgd --border-mode same --augment-mirror --activation relu \
    --epochs $EPOCHS --batch-size 32 --train "$TRAIN_DIR" --test "$TEST_DIR" --extension png \
    --learn-rate 0.1 --learn-momentum 0.9 --learn-anneal 0.5 --learn-anneal-epochs 15 30 45 60 75 --learn-decay 0.0005 \
    --model-desc $MODEL_DESC > train.out 2> train.err

$BIN/model-predict --model ./model_epoch$(printf "%03d" $((EPOCHS-1)))_final.mdl.gz --input "$TEST_DIR" --extension png \
    --batch-size 32 --predict-mode single
