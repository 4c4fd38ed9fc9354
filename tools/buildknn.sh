#!/bin/bash
# tools/buildknn.sh NAME [extra hipcc flags...]: build the KNN sources (knn.hip, knn_screen.hip,
# knn_merge.hip) with the extra flags and link them with every other product object (make first)
# as lib/libdsp_audiorec_NAME.so (KNN A/B variants)
set -e
n=$1; shift
make -C "$(dirname "$0")/../dsp-audioreclabs_amd/csrc" knnvariant V="$n" D="$*"
