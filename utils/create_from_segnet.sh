#!/bin/bash
# Labels from a trained SegNet-Basic snapshot for the 500 val images: N_GPUS background processes, contiguous image
# ranges of size n_data / N_GPUS + 1, one GPU each (the reference launcher of this name, its arguments and range split).
#   usage: bash utils/create_from_segnet.sh PARAM_DIR ITERATION IMG_ZIP_FN LABEL_ZIP_FN OUT_DIR N_GPUS [DTYPE] [SPLIT_PLANES] [LOADER_PROCS]
# DTYPE (an addition, default fp32): labels_from_segnet.py --dtype, fp32 or bf16.
# SPLIT_PLANES (an addition, 0 or 1, default 0): 1 appends labels_from_segnet.py --split_planes (DTYPE fp32 only).
# LOADER_PROCS (an addition, default 0): labels_from_segnet.py --loader_procs, decode workers PER PROCESS (the job needs
# N_GPUS x LOADER_PROCS CPUs for them).
PARAM_DIR=$1
ITERATION=$2
IMG_ZIP_FN=$3
LABEL_ZIP_FN=$4
OUT_DIR=$5
N_GPUS=${6:-1}
DTYPE=${7:-fp32}
SPLIT_PLANES=${8:-0}
LOADER_PROCS=${9:-0}
SPLIT_FLAG=
if [ "$SPLIT_PLANES" = "1" ]; then SPLIT_FLAG=--split_planes; fi
n_data=500
step=$(( n_data / N_GPUS + 1 ))
gpu=0
for (( s=0; s<n_data; s+=step )); do
    e=$(( s + step < n_data ? s + step : n_data ))
    HIP_VISIBLE_DEVICES=$gpu PYTHONWARNINGS=ignore python labels_from_segnet.py \
        --param_dir $PARAM_DIR --iteration $ITERATION --gpu 0 \
        --img_zip_fn $IMG_ZIP_FN --label_zip_fn $LABEL_ZIP_FN --out_dir $OUT_DIR \
        --start_index $s --end_index $e --eval_shape 1024 2048 --dtype $DTYPE $SPLIT_FLAG \
        --loader_procs $LOADER_PROCS &
    gpu=$(( gpu + 1 ))
done
wait
