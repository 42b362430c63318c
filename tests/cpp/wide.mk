# builds the device unit test of the one-point-per-wave group law (csrc/fu_wide.hpp):  make -C tests/cpp -f wide.mk
#   widetest  gfx950 only; run by tests/test_gpu_msm_wide.py on the GPU box
ROOT := ../..
all: widetest
widetest: widetest.hip $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp)
	/opt/rocm/bin/hipcc --offload-arch=gfx950 -O2 -Wno-unused-result -I $(ROOT)/crypto3-zk_amd/csrc widetest.hip -o $@
