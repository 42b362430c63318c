# builds the harness of the inner pairing product commitments:  make -C tests/cpp -f ipp2.mk
#   libipp2test.so  kzg_ipp2_hip::single / pair, pairing_inner_product_hip and the length checks over bls12_381 (ipp2_test.cpp, host compiler)
ROOT := ../..
SHIM_HDR := $(wildcard $(ROOT)/crypto3-zk_amd/include/nil/crypto3/zk/hip/*.hpp) $(ROOT)/include/zkhip.h
all: libipp2test.so
libipp2test.so: ipp2_test.cpp $(SHIM_HDR) $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp) $(ROOT)/crypto3-zk_amd/libzkhip.so
	g++ -std=c++17 -O2 -fPIC -pthread -shared -I $(ROOT)/crypto3-zk_amd/include -I $(ROOT)/include ipp2_test.cpp -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@
