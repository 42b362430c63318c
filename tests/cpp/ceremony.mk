# builds the harness of the setup ceremonies:  make -C tests/cpp -f ceremony.mk
#   libceremonytest.so  transform_accumulator, power_pairs / merge_pairs and contribute_randomness over bls12_381 / alt_bn128_254 (ceremony_test.cpp, host compiler)
ROOT := ../..
SHIM_HDR := $(wildcard $(ROOT)/crypto3-zk_amd/include/nil/crypto3/zk/hip/*.hpp) $(ROOT)/include/zkhip.h
all: libceremonytest.so
libceremonytest.so: ceremony_test.cpp $(SHIM_HDR) $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp) $(ROOT)/crypto3-zk_amd/libzkhip.so
	g++ -std=c++17 -O2 -fPIC -pthread -shared -I $(ROOT)/crypto3-zk_amd/include -I $(ROOT)/include ceremony_test.cpp -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@
