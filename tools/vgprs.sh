#!/bin/bash
# Register use of every raster (k_raster_blend and k_blend_order included), binning and setup kernel, of the depth-clip pre-pass and of
# the supersampled resolve, of the visibility counts, of the depth queries, of the delta reads, of the skinning kernels, of the morph kernel, of the item bounds, of the dual-quaternion skinning kernel, of the sparse morph kernel, of the computed-normals kernels and of the ray-cast kernels, for a set of -D flags:
# "SGPRs Spill" is the compiler's count of scalar registers parked in lanes of a VGPR (v_writelane / v_readlane code, no scratch): the
# raster kernels of the headline and of its colour variant have none.
# tools/vgprs.sh [-DSWR_...]   (run from anywhere; compiles swr_kernels.hip, swr_clip.hip, swr_resolve.hip, swr_count.hip,
# swr_depth_query.hip, swr_delta.hip, swr_skin.hip, swr_morph.hip, swr_item_bounds.hip, swr_skin_dq.hip, swr_morph_sparse.hip, swr_normals.hip and swr_rays.hip)
cd "$(dirname "$0")/../software-renderer_amd"
for src in csrc/swr_kernels.hip csrc/swr_clip.hip csrc/swr_resolve.hip csrc/swr_count.hip csrc/swr_depth_query.hip csrc/swr_delta.hip csrc/swr_skin.hip csrc/swr_morph.hip csrc/swr_item_bounds.hip csrc/swr_skin_dq.hip csrc/swr_morph_sparse.hip csrc/swr_normals.hip csrc/swr_rays.hip; do
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -fhip-fp32-correctly-rounded-divide-sqrt \
  -fno-fast-math -w "$@" -Rpass-analysis=kernel-resource-usage -c -o /tmp/vgprs_$$.o $src 2>&1 | python3 -c '
import re, sys
name = None
for l in sys.stdin:
    m = re.search(r"Function Name: (\S+)", l)
    if m: name = m.group(1); row = {}
    for k, pat in (("VGPRs", r"\sVGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                   ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        m = re.search(pat, l)
        if m and name: row[k] = int(m.group(1))
    if name and "LDS Size" in l and ("k_raster" in name or "k_blend" in name or "k_bin" in name or "k_setup" in name or "k_list_setup" in name or "k_clip" in name or "k_resolve" in name or "k_count" in name or "k_depth_tiles" in name or "k_depth_boxes" in name or "k_delta" in name or "k_skin" in name or "k_morph" in name or "k_item_bounds" in name or "_normals" in name or "k_rays" in name):
        import subprocess
        d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("swr::", "").replace("(swr::RasterArgs)", "").replace("(swr::BlendArgs)", "(BlendArgs)").replace("(anonymous namespace)::", "")
        print("%-50s VGPRs %3d  spill %2d  SGPRs Spill %2d  scratch %3d  waves/SIMD %d  static LDS %6d" % (d, row.get("VGPRs", -1), row.get("spill", 0), row.get("sspill", 0), row.get("scratch", 0), row.get("waves", 0), row.get("lds", 0)))
'
done
rm -f /tmp/vgprs_$$.o
