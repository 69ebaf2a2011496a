# Top-level build: HIP engine (gfx950 only), host front end, oracle (test infrastructure).
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
CLANGXX  ?= /opt/rocm/lib/llvm/bin/clang++   # acq_math.hpp uses clang vector types (ext_vector_type)
ARCH     := gfx950
PKG      := gnss-gps-sdr_amd
CSRC     := $(PKG)/csrc
HOST     := $(PKG)/host
LIBDIR   := $(PKG)/lib
BINDIR   := $(PKG)/bin
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function $(HIPFLAGS_EXTRA)
HOSTFLAGS:= -O2 -std=c++17 -fPIC -Wall -Wno-unknown-pragmas -ffp-contract=off

all: lib host oracle emul

lib: $(LIBDIR)/libgpsacq.so
$(LIBDIR)/libgpsacq.so: $(CSRC)/acq_kernels.hip $(CSRC)/key_kernels.hip $(CSRC)/iq_kernels.hip $(CSRC)/gen_kernels.hip $(CSRC)/track_kernels.hip $(CSRC)/track_iq_kernels.hip $(CSRC)/nav_kernels.hip $(CSRC)/obs_kernels.hip $(CSRC)/smooth_kernels.hip $(CSRC)/quality_kernels.hip $(CSRC)/fix_kernels.hip $(CSRC)/coarse_kernels.hip $(CSRC)/refine_kernels.hip $(CSRC)/snapq_kernels.hip $(CSRC)/doppler_kernels.hip $(CSRC)/aided_kernels.hip $(CSRC)/aided_iq_kernels.hip $(CSRC)/aided_coh_iq_kernels.hip $(CSRC)/snapshot_iq_kernels.hip $(CSRC)/snapq_iq_kernels.hip $(CSRC)/gpsacq_engine.cpp $(CSRC)/gpsacq_multi.cpp $(CSRC)/gpsacq_track.cpp $(CSRC)/gpsacq_nav.cpp $(CSRC)/*.hpp include/gpsacq.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/gpsacq_engine.cpp -o $(LIBDIR)/gpsacq_engine.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/gpsacq_multi.cpp -o $(LIBDIR)/gpsacq_multi.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/acq_kernels.hip -o $(LIBDIR)/acq_kernels.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/key_kernels.hip -o $(LIBDIR)/key_kernels.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/iq_kernels.hip -o $(LIBDIR)/iq_kernels.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/gen_kernels.hip -o $(LIBDIR)/gen_kernels.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/track_kernels.hip -o $(LIBDIR)/track_kernels.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/track_iq_kernels.hip -o $(LIBDIR)/track_iq_kernels.o
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/gpsacq_track.cpp -o $(LIBDIR)/gpsacq_track.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/nav_kernels.hip -o $(LIBDIR)/nav_kernels.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/obs_kernels.hip -o $(LIBDIR)/obs_kernels.o
	$(HIPCC) $(HIPFLAGS) -c $(CSRC)/smooth_kernels.hip -o $(LIBDIR)/smooth_kernels.o
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/quality_kernels.hip -o $(LIBDIR)/quality_kernels.o
	$(HIPCC) $(HIPFLAGS) -mllvm -disable-machine-licm -c $(CSRC)/fix_kernels.hip -o $(LIBDIR)/fix_kernels.o   # hoisted libm constants spill: see the file's head comment
	$(HIPCC) $(HIPFLAGS) -mllvm -disable-machine-licm -c $(CSRC)/coarse_kernels.hip -o $(LIBDIR)/coarse_kernels.o   # as fix_kernels.hip: see the file's head comment
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/refine_kernels.hip -o $(LIBDIR)/refine_kernels.o   # the NCO words are the host's to the bit
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/snapq_kernels.hip -o $(LIBDIR)/snapq_kernels.o   # lin and weight are the reference's to the bit
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -mllvm -disable-machine-licm -c $(CSRC)/doppler_kernels.hip -o $(LIBDIR)/doppler_kernels.o   # the NCO words as refine_kernels.hip; k_doppler_fix as coarse_kernels.hip
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/aided_kernels.hip -o $(LIBDIR)/aided_kernels.o   # the NCO words as refine_kernels.hip
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/aided_iq_kernels.hip -o $(LIBDIR)/aided_iq_kernels.o   # the NCO words as refine_kernels.hip
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/aided_coh_iq_kernels.hip -o $(LIBDIR)/aided_coh_iq_kernels.o   # the NCO words as refine_kernels.hip
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/snapshot_iq_kernels.hip -o $(LIBDIR)/snapshot_iq_kernels.o   # the NCO words as refine_kernels.hip
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/snapq_iq_kernels.hip -o $(LIBDIR)/snapq_iq_kernels.o   # lin and weight as snapq_kernels.hip
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $(CSRC)/gpsacq_nav.cpp -o $(LIBDIR)/gpsacq_nav.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIBDIR)/acq_kernels.o $(LIBDIR)/key_kernels.o $(LIBDIR)/iq_kernels.o $(LIBDIR)/gen_kernels.o $(LIBDIR)/track_kernels.o $(LIBDIR)/track_iq_kernels.o $(LIBDIR)/nav_kernels.o $(LIBDIR)/obs_kernels.o $(LIBDIR)/smooth_kernels.o $(LIBDIR)/quality_kernels.o $(LIBDIR)/fix_kernels.o $(LIBDIR)/coarse_kernels.o $(LIBDIR)/refine_kernels.o $(LIBDIR)/snapq_kernels.o $(LIBDIR)/doppler_kernels.o $(LIBDIR)/aided_kernels.o $(LIBDIR)/aided_iq_kernels.o $(LIBDIR)/aided_coh_iq_kernels.o $(LIBDIR)/snapshot_iq_kernels.o $(LIBDIR)/snapq_iq_kernels.o $(LIBDIR)/gpsacq_engine.o $(LIBDIR)/gpsacq_multi.o $(LIBDIR)/gpsacq_track.o $(LIBDIR)/gpsacq_nav.o -ldl -pthread

host: $(LIBDIR)/libgps_search.so $(BINDIR)/gps_test $(BINDIR)/gps_track $(BINDIR)/hip_floor $(BINDIR)/pk_fma_stream
# measurement aid of bench.py's roofline: the rate of a pure v_pk_fma_f32 stream on this box (roofline.pk_fma_stream_TF)
$(BINDIR)/pk_fma_stream: tools/ubench/pk_fma_stream.hip
	@mkdir -p $(BINDIR)
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ $<
# measurement aid of bench.py's e2e_cli leg: the wall clock of a HIP process that does nothing (runtime start-up floor)
$(BINDIR)/hip_floor: tools/ubench/hip_floor.hip
	@mkdir -p $(BINDIR)
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ $<
$(LIBDIR)/libgps_search.so: $(HOST)/search_api.cpp include/gps_search.h include/gpsacq.h $(LIBDIR)/libgpsacq.so
	$(CXX) $(HOSTFLAGS) -pthread -shared -o $@ $(HOST)/search_api.cpp -L$(LIBDIR) -lgpsacq -Wl,-rpath,'$$ORIGIN'
$(BINDIR)/gps_test: $(HOST)/gps_test.cpp include/gps_search.h $(LIBDIR)/libgps_search.so
	@mkdir -p $(BINDIR)
	$(CXX) $(HOSTFLAGS) -pthread -o $@ $(HOST)/gps_test.cpp -L$(LIBDIR) -lgps_search -lgpsacq -Wl,-rpath,'$$ORIGIN/../lib'

# offline tracking channels + NAV subframes (gpsacq_track*): our own front end, no reference counterpart on stdout
$(BINDIR)/gps_track: $(HOST)/gps_track.cpp include/gpsacq.h $(LIBDIR)/libgpsacq.so
	@mkdir -p $(BINDIR)
	$(CXX) $(HOSTFLAGS) -o $@ $(HOST)/gps_track.cpp -L$(LIBDIR) -lgpsacq -Wl,-rpath,'$$ORIGIN/../lib'

oracle:
	$(MAKE) -C oracle

emul: tests/emul/libemul_acq.so
# every source in tests/emul: emul_acq.cpp (the acquisition kernels' index math) and emul_spd.cpp (the solvers' Cholesky piece)
EMUL_SRC := $(wildcard tests/emul/*.cpp)
tests/emul/libemul_acq.so: $(EMUL_SRC) $(CSRC)/*.hpp
	$(CLANGXX) -x c++ $(HOSTFLAGS) -shared -o $@ $(EMUL_SRC)

# Drop-in check (authoring container only): the reference's own front end, compiled from where it lies and never copied,
# linked against our SearchInit/SearchTask.  The binary goes to oracle/_ref/ (git-ignored).  It travels to the GPU box for ONE
# consumer: tests/test_gpu_parity.py::test_reference_main_against_our_library, the only thing in the tree that opens it
# (`grep -rn gps_test_refmain`: that test, this target) -- no product path, bench.py and smoke() never touch it.
# It holds the reference's main() only (argument handling + the two calls); every search symbol it calls is ours.
dropin-check: $(LIBDIR)/libgps_search.so
	@mkdir -p oracle/_ref
	$(CXX) -O2 -I/root/reference/c /root/reference/c/test_search_offline.cpp -o oracle/_ref/gps_test_refmain \
	    -L$(LIBDIR) -lgps_search -lgpsacq -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

clean:
	rm -rf $(LIBDIR) $(BINDIR) build tests/emul/libemul_acq.so
	$(MAKE) -C oracle clean
.PHONY: all lib host oracle emul clean dropin-check
