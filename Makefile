# Build recipes.  The product is hbbft_amd/libhbtc.so (gfx950 HIP kernels + host C++ behind the
# C ABI of include/hbtc.h).  The kernel file is compiled once per kernel group (HBTC_PART=1..5)
# so the groups build in parallel (`make -j8 lib`); hbtc_rlc.hip (parts 6-7) and hbtc_msm.hip
# (parts 8-9) likewise.
#   hosttest : the kernel arithmetic headers compiled for the HOST (tests/native, test-only)
#   devtest  : the same headers behind a test-only device harness, once per Fq-product variant
#   oracle   : the C restatement of threshold_crypto (oracle/c, test + CPU-baseline only)
HIPCC ?= /opt/rocm/bin/hipcc
CLANGXX ?= /opt/rocm/lib/llvm/bin/clang++
CC ?= gcc
ARCH ?= gfx950
CSRC := hbbft_amd/csrc
HDRS := $(wildcard $(CSRC)/*.h) include/hbtc.h
BUILD := build
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -I$(CSRC)
PARTS := 1
RLC_PARTS := 6 7
MSM_PARTS := 8 9
SKG_PARTS := 10
KOBJS := $(foreach p,$(PARTS),$(BUILD)/hbtc_kernels.p$(p).o) $(foreach p,$(RLC_PARTS),$(BUILD)/hbtc_rlc.p$(p).o) \
         $(foreach p,$(MSM_PARTS),$(BUILD)/hbtc_msm.p$(p).o) $(foreach p,$(SKG_PARTS),$(BUILD)/hbtc_skg.p$(p).o) \
         $(BUILD)/hbtc_check.c1.o $(BUILD)/hbtc_check.c2.o $(BUILD)/hbtc_sig.s1.o $(BUILD)/hbtc_sig.s2.o $(BUILD)/hbtc_pb.o \
         $(BUILD)/hbtc_bcast.o $(BUILD)/hbtc_comb.o $(BUILD)/hbtc_enc.o $(BUILD)/hbtc_keygen.o $(BUILD)/hbtc_own.o \
         $(BUILD)/hbtc_sv.o $(BUILD)/hbtc_skgp.o
LIB := hbbft_amd/libhbtc.so

.PHONY: all lib hosttest devtest oracle clean resources roofline-constants
all: lib hosttest devtest oracle

lib: $(LIB)

# the one-block asm Fq product / squaring (generated; `make gen-fips` after editing the generator)
.PHONY: gen-fips
gen-fips:
	python3 tools/gen_fips_asm.py --selftest
	python3 tools/gen_fips_asm.py --selftest-lazy
	python3 tools/gen_fips_asm.py > $(CSRC)/fq_fips_asm.h
	python3 tools/gen_fips_asm.py --sr > $(CSRC)/fq_fips_sr.h
	python3 tools/gen_fq_rr.py --selftest-rr
	python3 tools/gen_fq_rr.py --selftest-w
	python3 tools/rr_bounds.py
	python3 tools/gen_fq_rr.py > $(CSRC)/fq_rr.h

$(BUILD):
	mkdir -p $(BUILD)

# decode, line tables, key-set tables, scalar multiplication: helpers inlined, the product as the
# shared subroutine (no stack frames: k_point_mul 1.5 KB -> 0, k_g2_steps 1.1 KB -> 264 B/lane)
$(BUILD)/hbtc_kernels.p%.o: $(CSRC)/hbtc_kernels.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=$* -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# part 6 (per-item G1 work) is built with every helper and the Fq product inlined: no calls
# (each call saves / restores live registers through scratch; 72.6 -> 67.9 ms per C3 launch).
# The shared-subroutine product (HBTC_FQMUL_SR) is 1.2 MB -> 150 KB of code here but no faster
# (isolated 48.5 vs 49.9 ms): the pass is VALU-issue-bound, not instruction-fetch-bound.
$(BUILD)/hbtc_rlc.p6.o: $(CSRC)/hbtc_rlc.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=6 -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@

# part 7 (k_rlc_tree, the tile sums) in an object of its own, so its product form and occupancy
# are chosen apart from the item kernels' (DESIGN.md §4 "The tile sums as a kernel of their own")
$(BUILD)/hbtc_rlc.p7.o: $(CSRC)/hbtc_rlc.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=7 -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@

$(BUILD)/hbtc_rlc.p%.o: $(CSRC)/hbtc_rlc.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=$* -c $< -o $@

# part 8 (G1 MSMs: the decryption combines) with every helper and the Fq product inlined: the
# bucket loop's mixed addition fits the instruction cache (k_msm_buckets 17.4 -> 15.1 ms per C3
# launch, k_msm_final 5.2 -> 4.3)
$(BUILD)/hbtc_msm.p8.o: $(CSRC)/hbtc_msm.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=8 -DHBTC_FQMUL_INLINE -DHBTC_INLINE_ALL -c $< -o $@

# part 9 (G2 MSMs: the signature combines past 64 shares) with helpers inlined and the product as
# the shared subroutine: no stack frames (k_msm_decode<Fq2> 1,008 -> 0 B/lane of scratch)
$(BUILD)/hbtc_msm.p9.o: $(CSRC)/hbtc_msm.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=9 -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

$(BUILD)/hbtc_msm.p%.o: $(CSRC)/hbtc_msm.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=$* -c $< -o $@

$(BUILD)/hbtc_skg.p%.o: $(CSRC)/hbtc_skg.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=$* -c $< -o $@

# the group checks in two translation units: the one-wave weighted passes (part 2) must not share
# the out-of-line GT helpers with the two-wave kernels (part 1)
# with the GT helpers (gt6.h mul / frob / exp_by_x) inlined: 960 -> ~330 B/lane of scratch (the
# by-reference operands of the calls went through the stack), C3 unchanged, the 125-ciphertext
# slice 18.3 -> 17.8 ms per epoch (profiles/r03/gt_inline/)
# with the Fq product / squaring as ONE shared subroutine each (HBTC_FQMUL_SR, fq_fips_sr.h):
# straight-line Fq2 products instead of the rolled select loop, ~100 B/lane less scratch; C3
# 11.35 -> 11.62 M shares/s (profiles/r03/fq_sr/)
$(BUILD)/hbtc_check.c%.o: $(CSRC)/hbtc_check.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_CHECK_PART=$* -DHBTC_GT_INLINE -DHBTC_FQMUL_SR -c $< -o $@

# the G2 item pass, all helpers inlined, the product as the shared subroutine (no ABI calls:
# C2 658k -> 696k, C4 3.67M -> 3.93M shares/s with the check kernels, profiles/r03/fq_sr/)
$(BUILD)/hbtc_sig.s2.o: $(CSRC)/hbtc_sig.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_SIG_PART=2 -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# the G2 decode half (k_sig_decode) with the product inlined: no scratch in its loops
# (588 -> 432 B/lane, the doubling loop's ~150 spilled dwords per bit gone)
$(BUILD)/hbtc_sig.s1.o: $(CSRC)/hbtc_sig.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_SIG_PART=1 -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@

# the pair-batch item pass (Ciphertext::verify / PublicKey::verify by RLC), helpers inlined,
# the product as the shared subroutine
$(BUILD)/hbtc_pb.o: $(CSRC)/hbtc_pb.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# the small combines (t <= 64: one workgroup per instance), helpers inlined, the product as the
# shared subroutine
$(BUILD)/hbtc_comb.o: $(CSRC)/hbtc_comb.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# PublicKey::encrypt (comb u, GLV r pk, pad, lane-pair w) and Fr polynomial evaluation: helpers
# inlined, the product as the shared subroutine (`make resources-enc` prints the resource report)
$(BUILD)/hbtc_enc.o: $(CSRC)/hbtc_enc.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# SyncKeyGen::generate + NetworkInfo::new (column sum, Fr interpolation, commitment evaluation by
# Horner): the flag set of hbtc_enc.o (`make resources-keygen` prints the resource report)
$(BUILD)/hbtc_keygen.o: $(CSRC)/hbtc_keygen.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# SecretKeyShare::sign (k_sig_share: cofactor clearing and the GLV multiplication by one secret
# scalar on lane pairs): the flag set of hbtc_enc.o (`make resources-own` prints the resource report)
$(BUILD)/hbtc_own.o: $(CSRC)/hbtc_own.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# signed messages grouped by signer (k_sv_items: cofactor clearing and two x-adic G2 multiplications
# per item on lane pairs; the signers' trees): the flag set of hbtc_enc.o (`make resources-sv` prints
# the resource report)
$(BUILD)/hbtc_sv.o: $(CSRC)/hbtc_sv.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# SyncKeyGen::new's Part and the Acks (k_skgp_commit, k_skgp_rows, k_skgp_vals: the stages in front of
# the encryption's): the flag set of hbtc_enc.o (`make resources-skgp` prints the resource report)
$(BUILD)/hbtc_skgp.o: $(CSRC)/hbtc_skgp.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# Reliable Broadcast: Reed-Solomon over GF(2^8), SHA3 Merkle trees and proofs
$(BUILD)/hbtc_bcast.o: $(CSRC)/hbtc_bcast.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/hbtc_api.o: $(CSRC)/hbtc_api.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/hbtc_hash.o: $(CSRC)/hbtc_hash.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $< -o $@

# host-only C++ over the public ABI (no device code)
$(BUILD)/hbtc_node.o: $(CSRC)/hbtc_node.cpp include/hbtc.h | $(BUILD)
	g++ -O2 -std=c++17 -fPIC -pthread -Wall -Iinclude -c $< -o $@

$(LIB): $(KOBJS) $(BUILD)/hbtc_api.o $(BUILD)/hbtc_hash.o $(BUILD)/hbtc_node.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@

# per-kernel VGPR / scratch / occupancy report (one part at a time: make resources PART=2)
PART ?= 2
resources:
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=$(PART) -c $(CSRC)/hbtc_kernels.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill"

# the DecryptionShare item pass (k_rlc_decode, k_rlc_rpk, k_rlc_items, k_rlc_tree) with its own flags
.PHONY: resources-rlc
resources-rlc:
	for p in 6 7; do $(HIPCC) $(HIPFLAGS) -DHBTC_PART=$$p -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE $(RLC_FLAGS) -c $(CSRC)/hbtc_rlc.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill|LDS"; done

# the MSM kernels (k_msm_buckets and its neighbours) with the flags of hbtc_msm.p8.o / p9.o;
# MSM_FLAGS=-DHBTC_MSM_WALK=0 reports the nested-loop walk, -DHBTC_FQ_RR=3 the walk on 12 x 32
.PHONY: resources-msm
resources-msm:
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=8 -DHBTC_FQMUL_INLINE -DHBTC_INLINE_ALL $(MSM_FLAGS) -c $(CSRC)/hbtc_msm.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill|LDS"
	$(HIPCC) $(HIPFLAGS) -DHBTC_PART=9 -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR $(MSM_FLAGS) -c $(CSRC)/hbtc_msm.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill|LDS"

.PHONY: resources-enc
resources-enc:
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $(CSRC)/hbtc_enc.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill"

# the SyncKeyGen producer's kernels, and hbtc_enc.hip again for k_enc_g1_rcpt beside k_enc_g1
.PHONY: resources-skgp
resources-skgp:
	for f in hbtc_skgp hbtc_enc; do $(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $(CSRC)/$$f.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill|LDS"; done

.PHONY: resources-keygen
resources-keygen:
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $(CSRC)/hbtc_keygen.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill|LDS"

.PHONY: resources-own
resources-own:
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $(CSRC)/hbtc_own.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill"

# the one-workgroup combines and the coin rounds' movers (k_coin_gather_pk, k_coin_final)
.PHONY: resources-comb
resources-comb:
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $(CSRC)/hbtc_comb.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill|LDS"

.PHONY: resources-sv
resources-sv:
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -c $(CSRC)/hbtc_sv.hip -o /dev/null \
	  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|AGPRs|Scratch|Occupancy|Spill|LDS"

hosttest: tests/native/libhbtc_hosttest.so tests/native/libhbtc_enc_hosttest.so tests/native/libhbtc_dec_hosttest.so \
          tests/native/libhbtc_keygen_hosttest.so tests/native/libhbtc_tree_hosttest.so \
          tests/native/libhbtc_own_hosttest.so tests/native/libhbtc_msm_hosttest.so \
          tests/native/libhbtc_rr_hosttest.so tests/native/libhbtc_rrw_hosttest.so \
          tests/native/libhbtc_xadicw_hosttest.so tests/native/libhbtc_msmw_hosttest.so \
          tests/native/libhbtc_skgp_hosttest.so
# skgp.h's host build (the SyncKeyGen producer's item bodies: the paired commitment, the triangle
# Horner, the Poly and FieldWrap frames)
tests/native/libhbtc_skgp_hosttest.so: tests/native/hbtc_skgp_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_skgp_hosttest.cpp -o $@
# the same as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU
.PHONY: sanitize-skgp
sanitize-skgp: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_skgp_host_main.cpp tests/native/hbtc_skgp_hosttest.cpp -o $(BUILD)/skgp_host_asan
	$(BUILD)/skgp_host_asan
# the 13 x 30 Fq code's host build (field.h FqR over fq_rr.h's plain 64-bit schedule, every MAD
# checked for a carry-out) and the G1 decode with its square root on it
tests/native/libhbtc_rr_hosttest.so: tests/native/hbtc_rr_hosttest.cpp tests/native/hbtc_rr_ops.h $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_rr_hosttest.cpp -o $@
# the same as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU
.PHONY: sanitize-rr
sanitize-rr: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_rr_host_main.cpp tests/native/hbtc_rr_hosttest.cpp -o $(BUILD)/rr_host_asan
	$(BUILD)/rr_host_asan
# the redundant 13 x 30 form's host build (field.h FqW, curve.h jacw_*: the |x| chains of
# k_rlc_decode's subgroup test), both bounds of every value tracked and asserted at every operation
tests/native/libhbtc_rrw_hosttest.so: tests/native/hbtc_rrw_hosttest.cpp tests/native/hbtc_rrw_ops.h $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_rrw_hosttest.cpp -o $@
# the same as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU
# (RRW_TABLE=file runs the case table tests/rrw_cases.py wrote and prints every result)
.PHONY: sanitize-rrw
sanitize-rrw: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_rrw_host_main.cpp tests/native/hbtc_rrw_hosttest.cpp -o $(BUILD)/rrw_host_asan
	$(BUILD)/rrw_host_asan $(RRW_TABLE)
# the item pass's x-adic multiplication on the redundant form (curve.h xadic_mul_sac8_w: the packed
# co-Z table chain, the column, the correction, the exit), both bounds tracked and asserted likewise
tests/native/libhbtc_xadicw_hosttest.so: tests/native/hbtc_xadicw_hosttest.cpp tests/native/hbtc_xadicw_ops.h $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_xadicw_hosttest.cpp -o $@
# the same as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU
# (XADICW_TABLE=file runs the case table tests/xadicw_cases.py wrote and prints every result)
.PHONY: sanitize-xadicw
sanitize-xadicw: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_xadicw_host_main.cpp tests/native/hbtc_xadicw_hosttest.cpp -o $(BUILD)/xadicw_host_asan
	$(BUILD)/xadicw_host_asan $(XADICW_TABLE)
# msm_walk.h's host build (one wave of the lane-uniform bucket walk in lockstep, over a toy group
# and over G1)
tests/native/libhbtc_msm_hosttest.so: tests/native/hbtc_msm_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_msm_hosttest.cpp -o $@
# the G1 bucket walk over JacW (k_msm_buckets<Fq> under HBTC_MSM_WALKW) in lockstep beside the 12 x 32
# walk, both bounds of every FqW tracked and asserted at every operation
tests/native/libhbtc_msmw_hosttest.so: tests/native/hbtc_msmw_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_msmw_hosttest.cpp -o $@
# the same as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU
.PHONY: sanitize-msm
sanitize-msm: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_msm_host_main.cpp tests/native/hbtc_msm_hosttest.cpp -o $(BUILD)/msm_host_asan
	$(BUILD)/msm_host_asan
# own_host.h's host build (the secret scalar of hbtc_decrypt_shares / hbtc_sign_shares: reduction,
# the x^2 split, the base-|x| digits, the wiping)
tests/native/libhbtc_own_hosttest.so: tests/native/hbtc_own_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_own_hosttest.cpp -o $@
# the same as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU
.PHONY: sanitize-own
sanitize-own: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_own_host_main.cpp tests/native/hbtc_own_hosttest.cpp -o $(BUILD)/own_host_asan
	$(BUILD)/own_host_asan
# rlc_tree.h's host build (the body of k_rlc_tree replayed merge by merge, every output against a
# plain restatement of the sums)
tests/native/libhbtc_tree_hosttest.so: tests/native/hbtc_tree_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_tree_hosttest.cpp -o $@
# the same as a stand-alone program under AddressSanitizer and UBSan: host code only, run on the CPU
.PHONY: sanitize-tree
sanitize-tree: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_tree_host_main.cpp tests/native/hbtc_tree_hosttest.cpp -o $(BUILD)/tree_host_asan
	$(BUILD)/tree_host_asan
tests/native/libhbtc_keygen_hosttest.so: tests/native/hbtc_keygen_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_keygen_hosttest.cpp -o $@
# keygen.h's host build (the column sum, the interpolation at 0 over its 256 simulated lanes, the
# Horner evaluation, the shared-inversion affine conversion) as a stand-alone program under
# AddressSanitizer and UBSan: host code only, run on the CPU
.PHONY: sanitize-keygen
sanitize-keygen: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_keygen_host_main.cpp tests/native/hbtc_keygen_hosttest.cpp -o $(BUILD)/keygen_host_asan
	$(BUILD)/keygen_host_asan
tests/native/libhbtc_dec_hosttest.so: tests/native/hbtc_dec_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_dec_hosttest.cpp -o $@
tests/native/libhbtc_enc_hosttest.so: tests/native/hbtc_enc_hosttest.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -I$(CSRC) tests/native/hbtc_enc_hosttest.cpp -o $@
# the decryption pad's host build (k_dec_seed + k_enc_pad bodies) as a stand-alone program under
# AddressSanitizer and UBSan: host code only, run on the CPU
.PHONY: sanitize-dec
sanitize-dec: | $(BUILD)
	$(CLANGXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) \
	  tests/native/hbtc_dec_host_main.cpp tests/native/hbtc_dec_hosttest.cpp -o $(BUILD)/dec_host_asan
	$(BUILD)/dec_host_asan
tests/native/libhbtc_hosttest.so: tests/native/hbtc_hosttest.cpp tests/native/gt_sim.cpp $(HDRS)
	$(CLANGXX) -O2 -std=c++17 -shared -fPIC -pthread -I$(CSRC) tests/native/hbtc_hosttest.cpp tests/native/gt_sim.cpp -o $@

# test-only device harness (tests/test_gpu_devarith.py): one object per variant of the Fq product,
# each with the flags of the product objects that use that variant; the kernels and entry points
# carry the variant's suffix, so the three link into one library
DEVTEST_OBJS := $(BUILD)/hbtc_devtest.sr.o $(BUILD)/hbtc_devtest.inl.o $(BUILD)/hbtc_devtest.call.o
$(BUILD)/hbtc_devtest.sr.o: tests/native/hbtc_devtest.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_SR -DHBTC_GT_INLINE -c $< -o $@
$(BUILD)/hbtc_devtest.inl.o: tests/native/hbtc_devtest.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@
$(BUILD)/hbtc_devtest.call.o: tests/native/hbtc_devtest.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
devtest: tests/native/libhbtc_devtest.so tests/native/libhbtc_tree_devtest.so tests/native/libhbtc_rr_devtest.so \
         tests/native/libhbtc_rrw_devtest.so tests/native/libhbtc_xadicw_devtest.so
# test-only device harness of the item pass's x-adic multiplication on the redundant form
# (tests/test_gpu_xadicw.py): hbtc_xadicw_ops.h on 64-lane workgroups with k_rlc_items' LDS layout,
# with the flags of hbtc_rlc.p6.o
$(BUILD)/rr_devtest/hbtc_xadicw_devtest.o: tests/native/hbtc_xadicw_devtest.hip tests/native/hbtc_xadicw_ops.h $(HDRS) | $(BUILD)
	mkdir -p $(BUILD)/rr_devtest
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@
tests/native/libhbtc_xadicw_devtest.so: $(BUILD)/rr_devtest/hbtc_xadicw_devtest.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@
# test-only device harness of the redundant 13 x 30 form (tests/test_gpu_rrw.py): the operations of
# hbtc_rrw_ops.h on one workgroup, with the flags of hbtc_rlc.p6.o
$(BUILD)/rr_devtest/hbtc_rrw_devtest.o: tests/native/hbtc_rrw_devtest.hip tests/native/hbtc_rrw_ops.h $(HDRS) | $(BUILD)
	mkdir -p $(BUILD)/rr_devtest
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@
tests/native/libhbtc_rrw_devtest.so: $(BUILD)/rr_devtest/hbtc_rrw_devtest.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@
# test-only device harness of the 13 x 30 Fq code (tests/test_gpu_rr.py): the operations of
# hbtc_rr_ops.h on one workgroup, with the flags of hbtc_rlc.p6.o; the object stays out of
# $(BUILD)/*.o, which tools/build_variant.sh links
$(BUILD)/rr_devtest/hbtc_rr_devtest.o: tests/native/hbtc_rr_devtest.hip tests/native/hbtc_rr_ops.h $(HDRS) | $(BUILD)
	mkdir -p $(BUILD)/rr_devtest
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@
tests/native/libhbtc_rr_devtest.so: $(BUILD)/rr_devtest/hbtc_rr_devtest.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@
tests/native/libhbtc_devtest.so: $(DEVTEST_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@
# test-only device harness of the tile tree (tests/test_gpu_rlc_tree.py): rlc_reduce_sp on one wave
# per tile beside the product's k_rlc_tree (the harness includes hbtc_rlc.hip), with the flags of
# hbtc_rlc.p6.o; the object stays out of $(BUILD)/*.o, which tools/build_variant.sh links
$(BUILD)/tree_devtest/hbtc_tree_devtest.o: tests/native/hbtc_tree_devtest.hip $(CSRC)/hbtc_rlc.hip $(HDRS) | $(BUILD)
	mkdir -p $(BUILD)/tree_devtest
	$(HIPCC) $(HIPFLAGS) -DHBTC_INLINE_ALL -DHBTC_FQMUL_INLINE -c $< -o $@
tests/native/libhbtc_tree_devtest.so: $(BUILD)/tree_devtest/hbtc_tree_devtest.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@

oracle: oracle/c/libtcoracle.so
oracle/c/libtcoracle.so: oracle/c/tc_oracle.c
	$(CC) -O3 -std=gnu11 -shared -fPIC -pthread $< -o $@

clean:
	rm -rf $(BUILD) tests/native/*.so hbbft_amd/*.so oracle/c/*.so

# Fqm per unit of work, measured on the kernels' own headers (host build, counting on)
roofline-constants: bench/roofline_constants.json
bench/roofline_constants.json: tools/fqm_count.cpp $(HDRS)
	mkdir -p bench build
	$(CLANGXX) -O1 -std=c++17 -DHBTC_COUNT_FQM -I$(CSRC) $< -o build/fqm_count
	build/fqm_count > $@
