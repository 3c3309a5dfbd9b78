# Builds the product library (HIP, gfx950 only) and the CPU oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC -Wall -Wno-unused-result --offload-arch=$(ARCH)
CSRC := dragonboat_amd/csrc
LIBDIR := dragonboat_amd/lib
LIB := $(LIBDIR)/libhipquorum.so
SRCS := $(CSRC)/hq_runtime.hip $(CSRC)/hq_commit.hip $(CSRC)/hq_commit_tiles.hip \
        $(CSRC)/hq_commit_lag.hip $(CSRC)/hq_bits.hip $(CSRC)/hq_ri_multi.hip $(CSRC)/hq_synth.hip \
        $(CSRC)/hq_ingest.hip $(CSRC)/hq_table.hip $(CSRC)/hq_pack.cpp $(CSRC)/hq_worker.cpp \
        $(CSRC)/hq_worker_host.cpp $(CSRC)/hq_worker_dev.cpp $(CSRC)/hq_worker_hb.cpp \
        $(CSRC)/hq_worker_lists.cpp $(CSRC)/hq_worker_lifecycle.cpp $(CSRC)/hq_pool.hip \
        $(CSRC)/hq_wire.cpp $(CSRC)/hq_stream.cpp $(CSRC)/hq_stream16.cpp $(CSRC)/hq_jobs.cpp $(CSRC)/hq_dstep.hip \
        $(CSRC)/hq_dstep_step.hip $(CSRC)/hq_dstep_layout.hip $(CSRC)/hq_dstep_run.hip \
        $(CSRC)/hq_engine.hip $(CSRC)/hq_wire_frame.cpp $(CSRC)/hq_wire_dev.hip \
        $(CSRC)/hq_heartbeat.hip $(CSRC)/hq_heartbeat_wire.hip $(CSRC)/hq_wire_frame_dev.hip \
        $(CSRC)/hq_config.hip $(CSRC)/hq_groups.hip $(CSRC)/hq_tick.hip \
        $(CSRC)/hq_worker_tick.cpp $(CSRC)/hq_hb_received.hip $(CSRC)/hq_worker_hbrecv.cpp
OBJS := $(patsubst $(CSRC)/%,$(LIBDIR)/%.o,$(basename $(SRCS)))
DEPS := $(wildcard $(CSRC)/*.h) include/hipquorum.h
CXX ?= g++
CXXFLAGS ?= -O3 -std=c++17 -fPIC -pthread -Wall -Wextra

all: $(LIB) oracle tools/link_probe

# the host-link probe bench.py's step legs run beside them (their link roofline)
tools/link_probe: tools/link_probe.cpp
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -o $@ $<

$(LIBDIR)/%.o: $(CSRC)/%.hip $(DEPS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# host-only sources (packers): plain C++
$(LIBDIR)/%.o: $(CSRC)/%.cpp $(DEPS)
	@mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -pthread -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle

# tuning variants (one library each, for A/B runs via HQ_LIB_PATH, tools/ab_libs.sh):
#   lib_ivN    records per lane of the table ingest kernels
#   lib_ingnostore / lib_ingnoload the grouped table ingest without its table stores / loads (timing probes: wrong output)
#   lib_engprof the engine's per-workgroup clocks and tile counts (hq_engine_wgprof; tools/engine_wgprof.py)
define variant
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) $(1) -shared -o $@ $(SRCS)
endef
tools/lib_iv%/libhipquorum.so: $(SRCS) $(DEPS)
	$(call variant,-DHQ_INGEST_V=$*)

clean:
	rm -rf $(LIBDIR) oracle/build

.PHONY: all oracle clean
tools/lib_ingnostore/libhipquorum.so: $(SRCS) $(DEPS)
	$(call variant,-DHQ_INGEST_NOSTORE)
tools/lib_ingnoload/libhipquorum.so: $(SRCS) $(DEPS)
	$(call variant,-DHQ_INGEST_NOLOAD)
tools/lib_engprof/libhipquorum.so: $(SRCS) $(DEPS)
	$(call variant,-DHQ_ENGINE_WGPROF)
# binned-ingest A/B (tools/ab_bin.sh): kernel parts removed (HQ_BIN_AB) or smaller regions
tools/lib_binab%/libhipquorum.so: $(SRCS) $(DEPS)
	$(call variant,-DHQ_BIN_AB=$*)
tools/lib_bintpb%/libhipquorum.so: $(SRCS) $(DEPS)
	$(call variant,-DHQ_BIN_TPB_SHIFT=$*)
# phase timestamps of the binned ingest (tools/binprof.hip includes hq_table.hip with HQ_BIN_PROF)
tools/binprof: tools/binprof.hip $(SRCS) $(DEPS) $(OBJS)
	$(HIPCC) $(HIPFLAGS) -c -o tools/binprof.o tools/binprof.hip
	$(HIPCC) $(HIPFLAGS) -pthread -o $@ tools/binprof.o $(filter-out $(LIBDIR)/hq_table.o,$(OBJS))
# persistent-engine experiments (tools/ab_engine.py): multi-batch loop / flat / claim kernels beside
# the engine, in a library of their own linked against the product library
tools/lib_engexp/libengexp.so: tools/engine_exp.hip $(LIB) $(DEPS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ tools/engine_exp.hip -L$(LIBDIR) -lhipquorum -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

