# TEST-ONLY host build of k1_sizes.h's rows for the cf32 kernels with statistics: cf32_stats_emul.cpp ->
# librpf_emul_cf32_stats.so, loaded by tests/test_cf32_stats.py.  A makefile of its own (make -f cf32_stats.mk), as
# cf32.mk: ROCm's clang compiles the file as HIP for the host alone (no device pass, no GPU code in the library, which is linked without the HIP runtime).
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_cf32_stats.so: cf32_stats_emul.cpp $(CSRC)/fft_core.h $(CSRC)/k1_sizes.h $(CSRC)/rpf_device_common.h
	$(CXX) -x hip --offload-host-only --rocm-path=/opt/rocm -O1 -std=c++17 -fPIC -ffp-contract=off -c -o cf32_stats_emul.host.o cf32_stats_emul.cpp
	$(CXX) -shared -o $@ cf32_stats_emul.host.o
	rm -f cf32_stats_emul.host.o
clean:
	rm -f librpf_emul_cf32_stats.so
.PHONY: clean
