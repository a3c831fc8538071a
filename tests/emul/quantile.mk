# TEST-ONLY host build of the per-bin quantiles over rtl-power-fftw_amd/csrc/quantile_core.h (the steps the kernels
# compile, walked in their pass order with the rows split over simulated workgroups): quantile_emul.cpp ->
# librpf_emul_quantile.so, loaded by tests/test_quantile.py.  A makefile of its own (make -f quantile.mk), as excise.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_quantile.so: quantile_emul.cpp $(CSRC)/quantile_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ quantile_emul.cpp
clean:
	rm -f librpf_emul_quantile.so
.PHONY: clean
