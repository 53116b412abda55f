#!/usr/bin/env python3
"""Build-time register / scratch check ("spills are HBM traffic").

The Makefile compiles every .hip with -Rpass-analysis=kernel-resource-usage and keeps the
remarks in build/<file>.res.  This script parses them and

  * FAILS (exit 1) when a kernel of the headline training step (config C2: pooled length bucket
    26, kernel size 19, and every non-templated stage kernel) has ScratchSize > 0 or any VGPR/SGPR
    spill -- a spilled hot kernel once cost 92 MB of scratch traffic per launch (r01);
  * prints every other kernel that spills (large-n / rare instantiations) as a warning;
  * with --table prints name, VGPRs, SGPRs, LDS, occupancy of the C2 step's kernels.

usage: check_resources.py build_dir [--table]
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occ", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
          "LDS Size [bytes/block]": "lds"}

# kernels one C2 training step launches (U = 300, k = 19, L = 200 -> n = 26, T = 1, B = 1024):
# demangled-name patterns.  Templated kernels are matched on their C2 instantiation.
C2_STEP = [
    r"^pack_tables_kernel", r"^conv_pool_mm_kernel<5, 2,",   # (input moments + BatchNorm1 fold inside conv_pool)
    r"^qmom_kernel<26>", r"^prep2_kernel<true>", r"^fc_fwd_bf_kernel<26, 2>",
    # the head backward's batch sums ride in the combiner launch (<1>: one task) and are finished in
    # passA (<26, 2>); <0>, head_bwd and <26, 0> are the same step with EXPLAINN_HEAD_PARTIALS=0
    r"^logits_bn_kernel<1>", r"^passA_kernel<26, 2>", r"^logits_bn_kernel<0>",
    r"^head_bwd_kernel<true, false>", r"^passA_kernel<26, 0>", r"^mid_fused_kernel", r"^passB_kernel<26>",
    r"^conv_bwd_mm_kernel<19>", r"^fin_bwd_kernel", r"adam_kernel",
]

# the input gradient (inputgrad.hip) at C2: an eval-mode attribution pass and a train step with dx
# launch these; held to the same no-spill rule
INPUT_GRAD = [
    r"^ig_eval_dy_kernel", r"^ig_coef_kernel", r"^ig_pair_kernel", r"^ig_tables_kernel",
    r"^input_grad_kernel<false, false>", r"^input_grad_kernel<true, false>", r"^input_grad_kernel<true, true>",
]
# in-silico mutagenesis (ism.hip) at C2: k = 19 -> four pooled windows per substitution, one task
ISM = [r"^ism_units_kernel<4>", r"^ism_sum_kernel<1>"]
# Integrated Gradients (pathgrad.hip): the path walk, the endpoint logits, the transposed convolution
PATHGRAD = [r"^pg_base_kernel", r"^pg_path_kernel", r"^pg_logits_kernel", r"^pg_gather_kernel"]
# device-side evaluation metrics (metrics.hip): every kernel of the sort, the scans and the reductions
METRICS = [
    r"^metrics_keys_binary_kernel", r"^metrics_keys_linear_kernel", r"^metrics_hist_kernel",
    r"^metrics_scatter_kernel", r"^metrics_scan_reduce_kernel<HistScan>", r"^metrics_scan_sums_kernel<HistScan>",
    r"^metrics_scan_apply_kernel<HistScan>", r"^metrics_scan_reduce_kernel<RunScan<true> >",
    r"^metrics_scan_sums_kernel<RunScan<true> >", r"^metrics_scan_apply_kernel<RunScan<true> >",
    r"^metrics_scan_reduce_kernel<RunScan<false> >", r"^metrics_scan_sums_kernel<RunScan<false> >",
    r"^metrics_scan_apply_kernel<RunScan<false> >", r"^metrics_binary_terms_kernel",
    r"^metrics_binary_final_kernel", r"^metrics_run_ends_kernel", r"^metrics_ranks_kernel",
    r"^metrics_sums_kernel", r"^metrics_means_kernel", r"^metrics_centred_kernel",
    r"^metrics_linear_final_kernel",
]
# tiled scan of a long sequence (scan.hip): the window staging and the unfold of the pooled track
SCAN = [r"^stage_windows_kernel", r"^scan_unfold_kernel"]
# variant effects (variants.hip): the staging of edited windows
VARIANTS = [r"^stage_edits_kernel"]
# haplotypes (haplotypes.hip): the staging of windows that carry a run of edits
HAPLOTYPES = [r"^stage_haplotypes_kernel"]
# dinucleotide-preserving shuffles (shuffle.hip): one lane per (row, shuffle), counters in LDS
SHUFFLE = [r"^dinuc_shuffle_kernel"]
# motif comparison (motifs.hip): the preparation and the all-pairs alignment search
MOTIFS = [r"^motif_prep_kernel", r"^motif_compare_kernel",
          # motif significance: column scores, histograms, range nulls, alignment p-values
          r"^motif_colscore_kernel", r"^motif_hist_kernel", r"^motif_null_kernel", r"^motif_pvalue_kernel"]
# motif tree (motiftree.hip): the quantisation, the one-workgroup agglomeration, the cut and the pooling
MOTIFTREE = [r"^motif_tree_prepare_kernel", r"^motif_tree_kernel", r"^motif_tree_cut_walk_kernel",
             r"^motif_tree_pool_kernel"]
# the activation null (actnull.hip): the LDS histogram and the tail / threshold scan
ACTNULL = [r"^act_hist_kernel", r"^act_null_kernel"]
# motif spacing (spacing.hip): the per-pair distance histogram and the binomial test
SPACING = [r"^spacing_hist_kernel", r"^spacing_test_kernel"]
# motif enrichment (enrich.hip): the per-record best site and the threshold test
ENRICH = [r"^record_best_kernel<true>", r"^record_best_kernel<false>", r"^enrich_test_kernel"]
# motif centrality (central.hip): the position histogram of best sites and the region test
CENTRAL = [r"^site_positions_kernel", r"^centrality_test_kernel"]
# the site callers (sites.hip: count / emit and the two scans; interpret.hip: maximum / count / accumulate
# of the filter -> PWM export and its scan)
SITES = [r"^sites_kernel<0>", r"^sites_kernel<1>", r"^sites_scan_tiles_kernel", r"^sites_scan_units_kernel",
         r"^site_kernel<0>", r"^site_kernel<1>", r"^site_kernel<2>", r"^site_scan_kernel"]
# known-motif sites (pwmsites.hip): the exact null and the count / emit scan (its two scans are SITES')
PWMSITES = [r"^pwm_null_kernel", r"^pwm_sites_kernel<0>", r"^pwm_sites_kernel<1>"]
# site q-values: the observed PWM score histogram (pwmsites.hip; dynamic LDS only, up to 160 KB: G rows of
# wmax bins + 2 bins, the tables, a tile's codes) and the BH table (siteq.hip; 4112 bytes of static LDS)
SITEQ = [r"^pwm_hist_kernel", r"^site_q_kernel"]
# known-motif enrichment (pwmbest.hip): the per-record best PWM site
PWMBEST = [r"^pwm_best_kernel"]
# variant effects on known motifs (pwmvariants.hip): the best ref / alt PWM site per (motif, variant)
PWMVARIANTS = [r"^pwm_variant_kernel"]
# word discovery (words.hip): presence counts (dynamic LDS: 4^k bits, 128 KiB at k = 10), the Fisher test and
# its arg-min, the sites pass
WORDS = [r"^word_count_kernel", r"^word_test_kernel", r"^word_pick_kernel", r"^word_sites_kernel"]
# greedy in-silico evolution (evolve.hip): one round's selection
EVOLVE = [r"^evolve_select_kernel"]
GATED = (C2_STEP + INPUT_GRAD + ISM + EVOLVE + PATHGRAD + METRICS + SCAN + VARIANTS + HAPLOTYPES + SHUFFLE + MOTIFS + MOTIFTREE + ACTNULL +
         SPACING + ENRICH + CENTRAL + SITES + PWMSITES + PWMBEST + SITEQ + PWMVARIANTS + WORDS)


# Register cliffs measured in the pipeline: 1024-thread blocks of which TWO must
# share a CU (300 units on 256 CUs take two rounds otherwise) -- 64 registers, not one more.
# passA: three waves per SIMD (512 registers / 3, in allocation units of 8).
# (mid_fused: the buckets up to 40, whose LDS lets two blocks share a CU; above, one block has the CU)
# conv_bwd_mm: five waves per SIMD (512 / 5 in units of 8), so that five four-wave workgroups share a CU
# and the C2 grid of 1216 is resident in one round.
# fc_fwd_bf, passB: five waves per SIMD, what their LDS images allow at the pooled length 26.
# conv_pool_mm<5, 2, true>: one wave per SIMD whatever it takes, but its total is set by BatchNorm1's
# auxiliary path, which may use what the filter bank leaves and no more (390 when the path moved in).
VGPR_CAP = {r"^mid_fused_kernel<([1-9]|[1-3]\d|40)>": 64, r"^prep2_kernel<true>": 64,
            r"^conv_pool_mm_kernel<5, 2, true>": 390,
            r"^passA_kernel<26, 0>": 168, r"^passA_kernel<26, 2>": 168,
            r"^conv_bwd_mm_kernel<19>": 96,
            r"^fc_fwd_bf_kernel<26, 2>": 96, r"^passB_kernel<26>": 96}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    return [re.sub(r"^void ", "", l.replace("(anonymous namespace)::", "").split("(")[0]) for l in out.splitlines()]


def parse(path):
    rows, cur = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1), "file": os.path.basename(path)[:-4]}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[FIELDS[m.group(1).strip()]] = int(m.group(2))
    return rows


def main():
    build = sys.argv[1]
    rows = []
    for f in sorted(glob.glob(os.path.join(build, "*.res"))):
        rows += parse(f)
    if not rows:
        print("check_resources: no *.res files under %s (build with the Makefile)" % build)
        return 1
    for r, name in zip(rows, demangle([r["mangled"] for r in rows])):
        r["name"] = name
    # what costs memory traffic: scratch and VGPR spills.  SGPR spills go to VGPR lanes
    # (v_writelane / v_readlane), no memory involved: reported in the table, not an error
    hard = lambda r: r.get("scratch", 0) > 0 or r.get("vgpr_spill", 0) > 0
    spilled = lambda r: hard(r) or r.get("sgpr_spill", 0) > 0
    hot = [r for r in rows if any(re.search(p, r["name"]) for p in GATED)]
    missing = [p for p in GATED if not any(re.search(p, r["name"]) for r in rows)]
    bad = [r for r in hot if hard(r)]
    others = [r for r in rows if spilled(r) and r not in hot]
    if "--table" in sys.argv:
        print("%-44s %5s %5s %7s %4s  %s" % ("kernel (C2 step)", "VGPR", "SGPR", "LDS", "occ", "scratch/spills"))
        for r in hot:
            print("%-44s %5d %5d %7d %4d  %d B/lane, %d sgpr, %d vgpr" % (
                r["name"][:44], r.get("vgpr", 0) + r.get("agpr", 0), r.get("sgpr", 0), r.get("lds", 0),
                r.get("occ", 0), r.get("scratch", 0), r.get("sgpr_spill", 0), r.get("vgpr_spill", 0)))
    # SGPR spills alone go to VGPR lanes (v_writelane), not to memory: counted, not listed
    for r in others:
        if r.get("scratch", 0) > 0:
            print("check_resources: note: %s (%s) uses scratch: %d B/lane, %d sgpr, %d vgpr spilled" % (
                r["name"], r["file"], r.get("scratch", 0), r.get("sgpr_spill", 0), r.get("vgpr_spill", 0)))
    rc = 0
    for r in rows:
        for pat, cap in VGPR_CAP.items():
            if re.search(pat, r["name"]) and r.get("vgpr", 0) + r.get("agpr", 0) > cap:
                print("check_resources: ERROR: %s uses %d registers, over its cap of %d (an occupancy step)"
                      % (r["name"], r.get("vgpr", 0) + r.get("agpr", 0), cap))
                rc = 1
    for p in missing:
        print("check_resources: ERROR: no kernel matches the C2-step pattern %r (renamed? update C2_STEP)" % p)
        rc = 1
    for r in bad:
        print("check_resources: ERROR: hot kernel %s (%s) spills: scratch %d B/lane, %d sgpr, %d vgpr" % (
            r["name"], r["file"], r.get("scratch", 0), r.get("sgpr_spill", 0), r.get("vgpr_spill", 0)))
        rc = 1
    print("check_resources: %d kernels, %d in the C2 step, %d of those spill; elsewhere %d use scratch, "
          "%d more spill SGPRs only" % (len(rows), len(hot), len(bad),
                                        sum(1 for r in others if r.get("scratch", 0) > 0),
                                        sum(1 for r in others if r.get("scratch", 0) == 0)))
    return rc


if __name__ == "__main__":
    sys.exit(main())
