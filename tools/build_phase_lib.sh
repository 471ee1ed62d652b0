#!/bin/bash
# builds tools/libafis_phase.so (or the path given as $1): the test library with -DAFIS_PHASE_TIMING in graph.hip / minu.hip (see tools/phase_probe.py)
set -e
OUT=$(realpath -m "${1:-$(dirname "$0")/libafis_phase.so}")
cd "$(dirname "$0")/../msu-latentafis_amd/csrc"
make -s -j8 libafis_hip.so libafis_hip_test.so
TMP=$(mktemp -d)
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -DAFIS_PHASE_TIMING -c graph.hip -o "$TMP/graph_ph.o"
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DAFIS_PHASE_TIMING -c minu.hip -o "$TMP/minu_ph.o"
hipcc --offload-arch=gfx950 -shared -fPIC adc.o adc_mfma.o adc_refine.o "$TMP/graph_ph.o" "$TMP/minu_ph.o" pq_encode.o gallery_edit.o gallery_subset.o afis_api.o afis_gallery.o afis_search.o afis_subset.o \
    template_io.o adc_direct.o afis_taps.o -o "$OUT"
rm -r "$TMP"
