# Build of the MI355X reduction engine (libnccl.so, C ABI of include/nccl.h) and of the CPU oracle.
#   make            -> nccl_amd/lib/libnccl.so  +  oracle/_build/liboracle.so
#   make lib        -> only the product library
#   make oracle     -> only the test oracle
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      := /opt/rocm/lib/llvm/bin/clang++
ARCH     ?= gfx950
BUILD    := build
LIBDIR   := nccl_amd/lib
SRCDIR   := nccl_amd/csrc

# -ffp-contract=off: never fuse x*s + acc into one FMA (PreMulSum parity).
# -fno-gpu-flush-denormals-to-zero: keep fp32 denormals like the reference (no -ftz, common.mk:103).
# EXTRA: extra defines for A/B builds of variants (e.g. EXTRA=-DNCCL_AMD_COPY_UNROLL=16 BUILD=build_ab LIBDIR=ablib/x)
EXTRA    ?=
COMMON   := -O3 -fPIC -std=c++17 -ffp-contract=off -fvisibility=hidden -Wall -Wno-unused-function \
            -Wno-unused-variable -Wno-unused-but-set-variable -Iinclude $(EXTRA)
HIPFLAGS := $(COMMON) --offload-arch=$(ARCH) -fno-gpu-flush-denormals-to-zero -munsafe-fp-atomics
HOSTSRC  := debug.cc bootstrap.cc ipc.cc transport.cc init.cc group.cc enqueue.cc p2p.cc rma.cc register.cc tuner.cc mapcheck.cc \
            devcomm.cc
HOSTOBJ  := $(HOSTSRC:%.cc=$(BUILD)/%.o)
DEVSRC   := $(notdir $(wildcard $(SRCDIR)/*.hip))
DEVOBJ   := $(DEVSRC:%.hip=$(BUILD)/%.o)
HDRS     := $(wildcard $(SRCDIR)/*.h) include/nccl.h include/nccl_device.h include/nccl_device_reduce_copy.h

all: lib oracle numerics-host bootstrap-test tuner-test nccl-perf comm-examples plan-test mapcheck-test xgmi-probe atomicity-probe \
     fp8-probe release-probe reuse-probe export-check-test barrier-probe bcast-plan-test bcast-example p2p-plan-test sendrecv-example \
     rma-plan-test sym-a2a-plan-test comm-split-test devapi-kernels devapi-layout-test devapi-example \
     devapi-rc-kernels devapi-rc-host-test devapi-rc-example

.PHONY: export-check-test
export-check-test: tests/native/export_check_test

lib: $(LIBDIR)/libnccl.so

$(BUILD)/%.o: $(SRCDIR)/%.cc $(HDRS)
	@mkdir -p $(BUILD)
	$(CXX) $(COMMON) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c $< -o $@

# The kernels' register / scratch / occupancy report goes to build/<name>.usage
# (tests/test_occupancy.py checks that every channel kernel fits two workgroups per CU).
$(BUILD)/%.o: $(SRCDIR)/%.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/$*.usage; \
	  st=$$?; grep -E "warning|error" $(BUILD)/$*.usage >&2; exit $$st

# -Wl,--version-script: export exactly nccl* / pnccl* (reference src/libnccl.map:13-19)
$(LIBDIR)/libnccl.so: $(HOSTOBJ) $(DEVOBJ) $(SRCDIR)/libnccl.map
	@mkdir -p $(LIBDIR)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -Wl,-soname,libnccl.so.2 -Wl,-Bsymbolic \
	  -Wl,--version-script=$(SRCDIR)/libnccl.map -o $@ $(HOSTOBJ) $(DEVOBJ) -lpthread -ldl
	ln -sf libnccl.so $(LIBDIR)/libnccl.so.2

oracle: oracle/_build/liboracle.so

oracle/_build/liboracle.so: oracle/nccl_oracle.c
	@mkdir -p oracle/_build
	gcc -O2 -fPIC -shared -fopenmp -ffp-contract=off -fno-fast-math -std=c11 -o $@ $< -lm

clean:
	rm -rf $(BUILD) $(LIBDIR) oracle/_build

.PHONY: all lib oracle clean

# test-only host build of the kernels' numerics, checked exhaustively against the oracle
numerics-host: build/libnumerics_host.so

build/libnumerics_host.so: tests/native/numerics_host.cc $(SRCDIR)/numerics.h
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -fPIC -shared -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ $<

.PHONY: numerics-host

# test-only host program exercising the TCP bootstrap across forked processes
bootstrap-test: build/bootstrap_test

build/bootstrap_test: tests/native/bootstrap_test.cc $(SRCDIR)/bootstrap.cc $(SRCDIR)/debug.cc $(HDRS)
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ tests/native/bootstrap_test.cc \
	  $(SRCDIR)/bootstrap.cc $(SRCDIR)/debug.cc -lpthread

.PHONY: bootstrap-test

# test-only tuner plugin (reference ABI v6) loaded through NCCL_TUNER_PLUGIN by the GPU tests
tuner-test: tests/native/libnccl-tuner-test.so

tests/native/libnccl-tuner-test.so: tests/native/tuner_plugin.c include/nccl_tuner.h include/nccl.h
	gcc -O2 -fPIC -shared -fvisibility=hidden -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ $<

.PHONY: tuner-test

# nccl-tests-style native driver written against include/nccl.h only (C ABI check + Python-free timing)
nccl-perf: tests/native/nccl_perf

tests/native/nccl_perf: tests/native/nccl_perf.cc include/nccl.h $(LIBDIR)/libnccl.so
	$(HIPCC) -O2 --offload-arch=$(ARCH) -Iinclude -o $@ $< -L$(LIBDIR) -lnccl -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

.PHONY: nccl-perf

# the reference's communicator-creation examples (pthread per rank, ncclCommInitAll) + a known-answer AllReduce
comm-examples: tests/native/comm_examples

tests/native/comm_examples: tests/native/comm_examples.cc include/nccl.h $(LIBDIR)/libnccl.so
	$(HIPCC) -O2 --offload-arch=$(ARCH) -Iinclude -o $@ $< -L$(LIBDIR) -lnccl -lpthread -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

.PHONY: comm-examples

# CU-driven peer bandwidth probe (run by bench.py's suite on multi-GPU nodes)
xgmi-probe: tests/native/xgmi_probe

tests/native/xgmi_probe: tests/native/xgmi_probe.hip
	$(HIPCC) -O2 --offload-arch=$(ARCH) -o $@ $<

.PHONY: xgmi-probe

# The host sources every CPU plan driver compiles (and their sanitizer twins under build/asan/), and the stubs the
# drivers share
PLANSRC  := $(SRCDIR)/enqueue.cc $(SRCDIR)/debug.cc
PLANDEPS := $(PLANSRC) $(wildcard tests/native/*.h) $(HDRS)
PLANCXX  := $(CXX) -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude

# CPU test driver of enqueue.cc's planning (no GPU: launches and the few HIP calls are stubbed)
plan-test: tests/native/plan_test

tests/native/plan_test: tests/native/plan_test.cc $(PLANDEPS)
	$(PLANCXX) -o $@ tests/native/plan_test.cc $(PLANSRC) -lpthread

.PHONY: plan-test

# CPU test driver of the Broadcast plan and of the partition its kernels walk (device_abi.h blockLenOf / sliceBounds /
# llPartBounds, called from both sides); stubs like plan_test's
bcast-plan-test: tests/native/bcast_plan_test

tests/native/bcast_plan_test: tests/native/bcast_plan_test.cc $(PLANDEPS)
	$(PLANCXX) -o $@ tests/native/bcast_plan_test.cc $(PLANSRC) -lpthread

.PHONY: bcast-plan-test

# a C-ABI caller of ncclBroadcast / ncclBcast written against include/nccl.h only (links with -lnccl alone)
bcast-example: tests/native/bcast_example

tests/native/bcast_example: tests/native/bcast_example.cc include/nccl.h $(LIBDIR)/libnccl.so
	$(HIPCC) -O2 --offload-arch=$(ARCH) -Iinclude -o $@ $< -L$(LIBDIR) -lnccl -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

.PHONY: bcast-example

# CPU test driver of the ncclSend / ncclRecv host plan (p2p.cc) and of the cut its kernel walks (device_abi.h p2pCut /
# p2pSteps / sliceBounds, called from both sides); launches and the few HIP calls are stubbed
p2p-plan-test: tests/native/p2p_plan_test

tests/native/p2p_plan_test: tests/native/p2p_plan_test.cc $(SRCDIR)/p2p.cc $(PLANDEPS)
	$(PLANCXX) -o $@ tests/native/p2p_plan_test.cc $(SRCDIR)/p2p.cc $(PLANSRC) -lpthread

.PHONY: p2p-plan-test

# CPU test driver of the ncclPutSignal / ncclSignal / ncclWaitSignal host plan and argument checks (rma.cc, group.cc);
# launches and the few HIP calls are stubbed
rma-plan-test: tests/native/rma_plan_test

tests/native/rma_plan_test: tests/native/rma_plan_test.cc $(SRCDIR)/rma.cc $(SRCDIR)/group.cc $(SRCDIR)/p2p.cc $(PLANDEPS)
	$(PLANCXX) -o $@ tests/native/rma_plan_test.cc $(SRCDIR)/rma.cc $(SRCDIR)/group.cc $(SRCDIR)/p2p.cc $(PLANSRC) -lpthread

.PHONY: rma-plan-test

# CPU sweep of the cut the zero-copy AlltoAll / Gather kernel walks (device_abi.h symA2ACut / symA2APart): a stand-alone
# host program, built under ASan+UBSan (host code only)
sym-a2a-plan-test: tests/native/sym_a2a_plan_test

tests/native/sym_a2a_plan_test: tests/native/sym_a2a_plan_test.cc $(SRCDIR)/device_abi.h
	$(CXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
	  -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

.PHONY: sym-a2a-plan-test

# a C-ABI caller of ncclSend / ncclRecv / ncclAlltoAll written against include/nccl.h only (links with -lnccl alone)
sendrecv-example: tests/native/sendrecv_example

tests/native/sendrecv_example: tests/native/sendrecv_example.cc include/nccl.h $(LIBDIR)/libnccl.so
	$(HIPCC) -O2 --offload-arch=$(ARCH) -Iinclude -o $@ $< -L$(LIBDIR) -lnccl -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

.PHONY: sendrecv-example

# The device API (include/nccl_device.h). Test kernels written against the two public headers only, driven
# through ctypes by tests/test_gpu_device_api.py; a CPU sweep of the header's pure functions (resource layout, teams,
# epoch compare), a stand-alone host program under ASan+UBSan; the reference's LSA AllReduce example restated against
# the C ABI, one pthread per rank (with a timing mode, profiles/README.md).
DEVAPIHDRS := include/nccl.h include/nccl_device.h include/nccl_device_reduce_copy.h
devapi-kernels: tests/native/libdevapi_kernels.so

tests/native/libdevapi_kernels.so: tests/native/devapi_kernels.hip $(DEVAPIHDRS) $(LIBDIR)/libnccl.so
	$(HIPCC) -O3 -std=c++17 -fPIC -shared -fvisibility=hidden --offload-arch=$(ARCH) -fno-gpu-flush-denormals-to-zero \
	  -ffp-contract=off -Iinclude -o $@ $< -L$(LIBDIR) -lnccl -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

devapi-layout-test: tests/native/devapi_layout_test

tests/native/devapi_layout_test: tests/native/devapi_layout_test.cc $(DEVAPIHDRS)
	$(CXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
	  -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

devapi-example: tests/native/devapi_example

tests/native/devapi_example: tests/native/devapi_example.hip $(DEVAPIHDRS) $(LIBDIR)/libnccl.so
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -Iinclude -o $@ $< -L$(LIBDIR) -lnccl -lpthread \
	  -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

.PHONY: devapi-kernels devapi-layout-test devapi-example

# The reduce-copy family of the device API (include/nccl_device_reduce_copy.h, DESIGN.md §2.7 "Reduce-copy"): its test
# kernels (tests/test_gpu_device_rc.py), built with the temporaries kept, so that the gfx950 assembly and the kernels'
# register / scratch report lie in build/devapi_rc/ (tests/test_device_rc_cpu.py reads both); a CPU sweep of ncclSymPtr
# and of the plan function, a stand-alone host program under ASan+UBSan; an LSA AllReduce written with the family, one
# pthread per rank, with devapi_example's timing mode.
RCBUILD := $(BUILD)/devapi_rc
devapi-rc-kernels: tests/native/libdevapi_rc_kernels.so

$(RCBUILD)/libdevapi_rc_kernels.so: tests/native/devapi_rc_kernels.hip $(DEVAPIHDRS) $(LIBDIR)/libnccl.so
	@mkdir -p $(RCBUILD)
	$(HIPCC) -O3 -std=c++17 -fPIC -shared -fvisibility=hidden --offload-arch=$(ARCH) -fno-gpu-flush-denormals-to-zero \
	  -ffp-contract=off -Iinclude -Rpass-analysis=kernel-resource-usage -save-temps=obj -o $@ $< -L$(LIBDIR) -lnccl \
	  -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)' 2> $(RCBUILD)/kernels.usage; \
	  st=$$?; grep -E "warning|error" $(RCBUILD)/kernels.usage >&2; exit $$st

tests/native/libdevapi_rc_kernels.so: $(RCBUILD)/libdevapi_rc_kernels.so
	cp $< $@

devapi-rc-host-test: tests/native/devapi_rc_host_test

tests/native/devapi_rc_host_test: tests/native/devapi_rc_host_test.cc $(DEVAPIHDRS)
	$(CXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
	  -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

devapi-rc-example: tests/native/devapi_rc_example

tests/native/devapi_rc_example: tests/native/devapi_rc_example.hip $(DEVAPIHDRS) $(LIBDIR)/libnccl.so
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -Iinclude -o $@ $< -L$(LIBDIR) -lnccl -lpthread \
	  -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

.PHONY: devapi-rc-kernels devapi-rc-host-test devapi-rc-example

# CPU test of ncclCommSplit / ncclCommShrink below the GPU: membership and inherited occupancy (split.h), the channel
# cap they feed (enqueue.cc, its launches stubbed) and the subset rounds and rendezvous of the bootstrap, ranks as threads
SPLITSRC := tests/native/comm_split_test.cc $(SRCDIR)/bootstrap.cc $(PLANSRC)
comm-split-test: build/comm_split_test

build/comm_split_test: $(SPLITSRC) $(PLANDEPS)
	@mkdir -p build
	$(PLANCXX) -o $@ $(SPLITSRC) -lpthread

.PHONY: comm-split-test

# Host sanitizer builds (SURVEY §5 race detection; tests/test_sanitizers.py): the bootstrap, the IPC fd server
# and the planning code under ASan+UBSan and, separately, TSan. Host code only — no GPU code is instrumented.
SANCXX   := $(CXX) -g -O1 -fno-omit-frame-pointer -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude
ASAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined
TSAN     := -fsanitize=thread
HIPRT    := -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
SANBIN   := build/asan/bootstrap_test build/asan/plan_test build/asan/ipc_server_test \
            build/tsan/bootstrap_test build/tsan/ipc_server_test build/asan/bcast_plan_test build/asan/p2p_plan_test \
            build/asan/rma_plan_test build/asan/comm_split_test build/tsan/comm_split_test
sanitize: $(SANBIN)

build/asan/comm_split_test build/tsan/comm_split_test: $(SPLITSRC) $(PLANDEPS)
	@mkdir -p $(dir $@)
	$(SANCXX) $(if $(findstring asan,$@),$(ASAN),$(TSAN)) -o $@ $(SPLITSRC) -lpthread

build/asan/bootstrap_test build/tsan/bootstrap_test: tests/native/bootstrap_test.cc $(SRCDIR)/bootstrap.cc $(SRCDIR)/debug.cc $(HDRS)
	@mkdir -p $(dir $@)
	$(SANCXX) $(if $(findstring asan,$@),$(ASAN),$(TSAN)) -o $@ tests/native/bootstrap_test.cc $(SRCDIR)/bootstrap.cc \
	  $(SRCDIR)/debug.cc -lpthread

build/asan/ipc_server_test build/tsan/ipc_server_test: tests/native/ipc_server_test.cc $(SRCDIR)/ipc.cc $(SRCDIR)/debug.cc $(HDRS)
	@mkdir -p $(dir $@)
	$(SANCXX) $(if $(findstring asan,$@),$(ASAN),$(TSAN)) -o $@ tests/native/ipc_server_test.cc $(SRCDIR)/ipc.cc \
	  $(SRCDIR)/debug.cc -lpthread $(HIPRT)

# CPU test of the stale dma-buf export checks (ipc.cc ipcAdmitExport) with memfd files in place of dma-bufs
tests/native/export_check_test: tests/native/export_check_test.cc $(SRCDIR)/ipc.cc $(SRCDIR)/debug.cc $(HDRS)
	$(CXX) -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ tests/native/export_check_test.cc \
	  $(SRCDIR)/ipc.cc $(SRCDIR)/debug.cc -lpthread $(HIPRT)

build/asan/bcast_plan_test: tests/native/bcast_plan_test.cc $(PLANDEPS)
	@mkdir -p $(dir $@)
	$(SANCXX) $(ASAN) -o $@ tests/native/bcast_plan_test.cc $(PLANSRC) -lpthread

build/asan/p2p_plan_test: tests/native/p2p_plan_test.cc $(SRCDIR)/p2p.cc $(PLANDEPS)
	@mkdir -p $(dir $@)
	$(SANCXX) $(ASAN) -o $@ tests/native/p2p_plan_test.cc $(SRCDIR)/p2p.cc $(PLANSRC) -lpthread

build/asan/rma_plan_test: tests/native/rma_plan_test.cc $(SRCDIR)/rma.cc $(SRCDIR)/group.cc $(SRCDIR)/p2p.cc $(PLANDEPS)
	@mkdir -p $(dir $@)
	$(SANCXX) $(ASAN) -o $@ tests/native/rma_plan_test.cc $(SRCDIR)/rma.cc $(SRCDIR)/group.cc $(SRCDIR)/p2p.cc $(PLANSRC) -lpthread

build/asan/plan_test: tests/native/plan_test.cc $(PLANDEPS)
	@mkdir -p $(dir $@)
	$(SANCXX) $(ASAN) -o $@ tests/native/plan_test.cc $(PLANSRC) -lpthread

.PHONY: sanitize

# store-atomicity probe (torn 8/16/64/128-byte lines under concurrent write-through stores; GPU test + bench suite)
atomicity-probe: tests/native/store_atomicity_probe

tests/native/store_atomicity_probe: tests/native/store_atomicity_probe.hip
	$(HIPCC) -O3 --offload-arch=$(ARCH) -o $@ $<

.PHONY: atomicity-probe

# fp8 conversion probe: gfx950's fp8 convert instructions vs numerics.h's software conversions, every code and
# every half value (GPU test tests/test_gpu_numerics.py; decides the hardware fp8 path)
fp8-probe: tests/native/fp8_cvt_probe tests/native/fp8_f16_probe

tests/native/fp8_f16_probe: tests/native/fp8_f16_probe.hip $(SRCDIR)/numerics.h
	$(HIPCC) -O3 --offload-arch=$(ARCH) -ffp-contract=off -fno-gpu-flush-denormals-to-zero -o $@ $<

tests/native/fp8_cvt_probe: tests/native/fp8_cvt_probe.hip $(SRCDIR)/numerics.h
	$(HIPCC) -O3 --offload-arch=$(ARCH) -ffp-contract=off -fno-gpu-flush-denormals-to-zero -o $@ $<

.PHONY: fp8-probe

# CPU test driver of the init-time mapping check (mapcheck.cc) with the device and the imports stubbed
mapcheck-test: tests/native/mapcheck_test

tests/native/mapcheck_test: tests/native/mapcheck_test.cc $(SRCDIR)/mapcheck.cc $(SRCDIR)/debug.cc $(HDRS)
	$(CXX) -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ tests/native/mapcheck_test.cc \
	  $(SRCDIR)/mapcheck.cc $(SRCDIR)/debug.cc -lpthread

.PHONY: mapcheck-test

# does a kernel queued behind another on the same stream start while the first is resident?
barrier-probe: tests/native/barrier_probe

tests/native/barrier_probe: tests/native/barrier_probe.hip
	$(HIPCC) -O2 --offload-arch=$(ARCH) -o $@ $<

.PHONY: barrier-probe

# does unmapping an imported dma-buf mapping wait for the device? (decides where peers' mappings are released,
# DESIGN.md §3.2)
release-probe: tests/native/release_probe

tests/native/release_probe: tests/native/release_probe.hip
	$(HIPCC) -O2 --offload-arch=$(ARCH) -o $@ $<

.PHONY: release-probe

# the importer's unmap-then-allocate pattern of eager registration churn, without the library
reuse-probe: tests/native/reuse_probe

tests/native/reuse_probe: tests/native/reuse_probe.hip
	$(HIPCC) -O2 --offload-arch=$(ARCH) -o $@ $<

.PHONY: reuse-probe
