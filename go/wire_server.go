// wire_server.go — the payload stage behind the gRPC server: the handler registered in V1_ServiceDesc's place never unmarshals, it hands the
// bytes of the GetRateLimitsReq to guber_wire_pool_get_rate_limits and returns the bytes of the GetRateLimitsResp (include/guber_wire.h,
// INTEGRATION.md section 3g).  What it replaces: _V1_GetRateLimits_Handler (gubernator_grpc.pb.go:111-127) + V1Instance.GetRateLimits
// (gubernator.go:183-306) for requests this instance owns; _PeersV1_GetPeerRateLimits_Handler (peers_grpc.pb.go:109) +
// V1Instance.GetPeerRateLimits (gubernator.go:462-539) through guber_wire_pool_get_peer_rate_limits; _PeersV1_UpdatePeerGlobals_Handler +
// V1Instance.UpdatePeerGlobals (gubernator.go:425-459) through guber_wire_pool_update_peer_globals.
//
// NOT compiled in this repository (no Go toolchain in the build image): the calls below are made, in the same order and with the same
// arguments, by tests/hostsim/abi_c99.c (wire_pool_sequence) and tests/hostsim/peer_abi_c99.c (the two peer handlers) — compiled as C99
// against the public headers and run on the GPU; MeshWireServer's by tests/hostsim/mesh_pool_abi_c99.c.
package gubernator

/*
#cgo CFLAGS: -I${SRCDIR}/../include
#cgo LDFLAGS: -L${SRCDIR}/../gubernator_amd -lguber_hip
#include <stdlib.h>
#include "guber_gpu.h"
#include "guber_wire.h"
*/
import "C"

import (
	"context"
	"sync/atomic"
	"unsafe"

	"google.golang.org/grpc"
	"google.golang.org/grpc/codes"
	"google.golang.org/grpc/status"
	"google.golang.org/protobuf/proto"
)

// rawMessage is a message that IS its bytes; rawCodec leaves it alone (grpc.ForceServerCodec(rawCodec{}) on the servers of daemon.go:119-144).
// Everything else — HealthCheck keeps its generated handler, and so does any method a daemon does not hand to the payload stage — is a
// generated message and goes through the protobuf runtime as under the default codec.
type rawMessage struct{ b []byte }
type rawCodec struct{}

func (rawCodec) Marshal(v interface{}) ([]byte, error) {
	if m, ok := v.(*rawMessage); ok {
		return m.b, nil
	}
	return proto.Marshal(v.(proto.Message))
}
func (rawCodec) Unmarshal(d []byte, v interface{}) error {
	if m, ok := v.(*rawMessage); ok {
		m.b = d
		return nil
	}
	return proto.Unmarshal(d, v.(proto.Message))
}
func (rawCodec) Name() string { return "proto" }

// WireServer owns the payload stage of ONE device.
type WireServer struct {
	pool *C.guber_wire_pool_t
}

// NewWireServer: the engines of the device (GPUWorkerPool's shards), the placement's rule (nil with one table), the defaults of
// guber_wire_pool_config_t (twelve stages of 49 152 items, BatchWait 500 us, 1000 requests per RPC).
func NewWireServer(engines []*C.guber_engine_t, rule *C.struct_guber_route_rule) (*WireServer, error) {
	s := &WireServer{}
	if rc := C.guber_wire_pool_create(&engines[0], C.uint32_t(len(engines)), rule, nil, &s.pool); rc != C.GUBER_OK {
		return nil, status.Errorf(codes.Internal, "guber_wire_pool_create: %s", C.GoString(C.guber_last_error()))
	}
	return s, nil
}

// Close: no call may be in flight or arrive any more (the gRPC servers have been stopped: daemon.go Close).
func (s *WireServer) Close() { C.guber_wire_pool_destroy(s.pool) }

// call hands one serialized message over and returns the serialized answer.  peer: the message is a GetPeerRateLimitsReq and is answered as
// V1Instance.GetPeerRateLimits answers it (no validation, DRAIN_OVER_LIMIT on forwarded GLOBAL items, its error texts); otherwise the client
// RPC with the error texts of gubernator.go:250-255.
func (s *WireServer) call(in []byte, peer bool) ([]byte, error) {
	if len(in) == 0 {
		return nil, nil // no requests: an empty GetRateLimitsResp
	}
	p := (*C.uint8_t)(unsafe.Pointer(&in[0]))
	out := make([]byte, int(C.guber_wire_pool_response_bound(p, C.size_t(len(in)))))
	var n C.size_t
	// blocks (a cgo call: the goroutine keeps its thread) until the stage the payload joined has been through the GPU
	var rc C.int
	if peer {
		rc = C.guber_wire_pool_get_peer_rate_limits(s.pool, p, C.size_t(len(in)), (*C.uint8_t)(unsafe.Pointer(&out[0])), C.size_t(len(out)), &n)
	} else {
		rc = C.guber_wire_pool_get_rate_limits(s.pool, p, C.size_t(len(in)), 1, 1, (*C.uint8_t)(unsafe.Pointer(&out[0])), C.size_t(len(out)), &n)
	}
	switch rc {
	case C.GUBER_OK:
		return out[:int(n)], nil
	case C.GUBER_E_WIRE_TOO_LARGE:
		if peer { // gubernator.go:464-467
			return nil, status.Errorf(codes.OutOfRange, "'PeerRequest.rate_limits' list too large; max size is '%d'", maxBatchSize)
		}
		// gubernator.go:189-193
		return nil, status.Errorf(codes.OutOfRange, "Requests.RateLimits list too large; max size is '%d'", maxBatchSize)
	case C.GUBER_E_WIRE_MALFORMED: // what protobuf-go's Unmarshal failure becomes in grpc-go
		return nil, status.Error(codes.Internal, "grpc: error unmarshalling request")
	default:
		return nil, status.Errorf(codes.Internal, "guber_wire_pool: %s", C.GoString(C.guber_last_error()))
	}
}

// The method handlers, with the signature grpc.MethodDesc.Handler wants (gubernator_grpc.pb.go:150-165, peers_grpc.pb.go:148-163).
func (s *WireServer) getRateLimits(_ interface{}, _ context.Context, dec func(interface{}) error, _ grpc.UnaryServerInterceptor) (interface{}, error) {
	in := new(rawMessage)
	if err := dec(in); err != nil {
		return nil, err
	}
	out, err := s.call(in.b, false)
	return &rawMessage{out}, err
}

func (s *WireServer) getPeerRateLimits(_ interface{}, _ context.Context, dec func(interface{}) error, _ grpc.UnaryServerInterceptor) (interface{}, error) {
	in := new(rawMessage)
	if err := dec(in); err != nil {
		return nil, err
	}
	out, err := s.call(in.b, true)
	return &rawMessage{out}, err
}

// updatePeerGlobals: the owner's broadcast of GLOBAL buckets (raw bytes in), installed where the pool keeps GLOBAL state; the answer is the
// empty UpdatePeerGlobalsResp (gubernator.go:458).
func (s *WireServer) updatePeerGlobals(_ interface{}, _ context.Context, dec func(interface{}) error, _ grpc.UnaryServerInterceptor) (interface{}, error) {
	in := new(rawMessage)
	if err := dec(in); err != nil {
		return nil, err
	}
	if len(in.b) == 0 {
		return &rawMessage{}, nil // no globals
	}
	var installed C.uint32_t
	switch rc := C.guber_wire_pool_update_peer_globals(s.pool, (*C.uint8_t)(unsafe.Pointer(&in.b[0])), C.size_t(len(in.b)), &installed); rc {
	case C.GUBER_OK:
		return &rawMessage{}, nil
	case C.GUBER_E_WIRE_MALFORMED:
		return nil, status.Error(codes.Internal, "grpc: error unmarshalling request")
	default: // gubernator.go:452-455
		return nil, status.Errorf(codes.Internal, "Error in workerPool.AddCacheItem: %s", C.GoString(C.guber_last_error()))
	}
}

// ServiceDescs: V1_ServiceDesc / PeersV1_ServiceDesc with GetRateLimits, GetPeerRateLimits and UpdatePeerGlobals replaced (HealthCheck keeps its
// generated handler: rawCodec hands generated messages to the protobuf runtime).
func (s *WireServer) ServiceDescs() (grpc.ServiceDesc, grpc.ServiceDesc) {
	v1, peers := V1_ServiceDesc, PeersV1_ServiceDesc
	v1.Methods = append([]grpc.MethodDesc(nil), v1.Methods...)
	peers.Methods = append([]grpc.MethodDesc(nil), peers.Methods...)
	for i := range v1.Methods {
		if v1.Methods[i].MethodName == "GetRateLimits" {
			v1.Methods[i].Handler = s.getRateLimits
		}
	}
	for i := range peers.Methods {
		if peers.Methods[i].MethodName == "GetPeerRateLimits" {
			peers.Methods[i].Handler = s.getPeerRateLimits
		}
		if peers.Methods[i].MethodName == "UpdatePeerGlobals" {
			peers.Methods[i].Handler = s.updatePeerGlobals
		}
	}
	return v1, peers
}

// MeshWireServer owns the payload stage over a MESH (guber_wire_mesh_pool_*, INTEGRATION.md section 3h): one daemon in front of several GPUs,
// every GPU a rank of a guber_mesh_t and a peer of the ring.  The handler hands the bytes of the GetRateLimitsReq to ANY rank; the ring's owner
// decision (gubernator.go:236-283), the evaluation on the owner and the marshalling — with metadata{"owner": <address>} on every answer another
// rank owns — happen on the devices.  GetPeerRateLimits and UpdatePeerGlobals are not served here: every peer of the ring is a local rank.
type MeshWireServer struct {
	pool  *C.guber_wire_mesh_pool_t
	ranks uint32
	next  uint32 // the rank the next RPC arrives at: round robin
	addrs []*C.char
}

// NewMeshWireServer: the mesh (the daemon keeps it, its fronts and their engines, and destroys them after Close), the ring's peer names —
// ownerAddr[r] is the address peer r was given in guber_ring_create — and the defaults of guber_wire_mesh_pool_config_t with the error texts
// of gubernator.go:250-255.
func NewMeshWireServer(mesh *C.guber_mesh_t, ownerAddr []string) (*MeshWireServer, error) {
	s := &MeshWireServer{ranks: uint32(len(ownerAddr))}
	for _, a := range ownerAddr {
		s.addrs = append(s.addrs, C.CString(a))
	}
	var cfg C.guber_wire_mesh_pool_config_t
	cfg.wrap_errors = 1
	if rc := C.guber_wire_mesh_pool_create(mesh, &s.addrs[0], &cfg, &s.pool); rc != C.GUBER_OK {
		s.free()
		return nil, status.Errorf(codes.Internal, "guber_wire_mesh_pool_create: %s", C.GoString(C.guber_last_error()))
	}
	return s, nil
}

// SetDirect: lone small RPCs evaluated by their handler's own thread (guber_wire_mesh_pool_set_direct) — RPCs of at most maxItems items
// (0 = off, the default; at most 256) while at most maxCalls calls (0 = 8) are inside the pool take the mesh's one-launch call instead of a
// stage set.  May be called while the server runs.
func (s *MeshWireServer) SetDirect(maxItems, maxCalls uint32) error {
	if rc := C.guber_wire_mesh_pool_set_direct(s.pool, C.uint32_t(maxItems), C.uint32_t(maxCalls)); rc != C.GUBER_OK {
		return status.Errorf(codes.InvalidArgument, "guber_wire_mesh_pool_set_direct: %s", C.GoString(C.guber_last_error()))
	}
	return nil
}

// DirectStats: RPCs served by their callers so far, and those of them whose small call met a fall-back.
func (s *MeshWireServer) DirectStats() (direct, fallbacks uint64) {
	var st C.guber_wire_mesh_pool_direct_stats_t
	C.guber_wire_mesh_pool_direct_stats(s.pool, &st)
	return uint64(st.direct_rpcs), uint64(st.fallback_rpcs)
}

func (s *MeshWireServer) free() {
	for _, a := range s.addrs {
		C.free(unsafe.Pointer(a))
	}
	s.addrs = nil
}

// Close: no call may be in flight or arrive any more (the gRPC servers have been stopped); before the mesh is destroyed.
func (s *MeshWireServer) Close() {
	C.guber_wire_mesh_pool_destroy(s.pool)
	s.free()
}

// getRateLimitsMeshRaw: the GetRateLimits handler over the mesh (the signature grpc.MethodDesc.Handler wants).  rank = a counter modulo the
// ranks; the buffer is guber_wire_mesh_pool_response_bound's, so nothing is ever found too small after decisions have been applied.
func (s *MeshWireServer) getRateLimitsMeshRaw(_ interface{}, _ context.Context, dec func(interface{}) error, _ grpc.UnaryServerInterceptor) (interface{}, error) {
	in := new(rawMessage)
	if err := dec(in); err != nil {
		return nil, err
	}
	if len(in.b) == 0 {
		return &rawMessage{}, nil // no requests: an empty GetRateLimitsResp
	}
	rank := C.uint32_t((atomic.AddUint32(&s.next, 1) - 1) % s.ranks)
	p := (*C.uint8_t)(unsafe.Pointer(&in.b[0]))
	out := make([]byte, int(C.guber_wire_mesh_pool_response_bound(s.pool, p, C.size_t(len(in.b)))))
	var n C.size_t
	// blocks (a cgo call: the goroutine keeps its thread) until the stage set the payload joined has been through the GPUs
	switch rc := C.guber_wire_mesh_pool_get_rate_limits(s.pool, rank, p, C.size_t(len(in.b)), (*C.uint8_t)(unsafe.Pointer(&out[0])), C.size_t(len(out)), &n); rc {
	case C.GUBER_OK:
		return &rawMessage{out[:int(n)]}, nil
	case C.GUBER_E_WIRE_TOO_LARGE: // gubernator.go:189-193
		return nil, status.Errorf(codes.OutOfRange, "Requests.RateLimits list too large; max size is '%d'", maxBatchSize)
	case C.GUBER_E_WIRE_MALFORMED: // what protobuf-go's Unmarshal failure becomes in grpc-go
		return nil, status.Error(codes.Internal, "grpc: error unmarshalling request")
	default:
		return nil, status.Errorf(codes.Internal, "guber_wire_mesh_pool: %s", C.GoString(C.guber_last_error()))
	}
}

// ServiceDesc: V1_ServiceDesc with GetRateLimits replaced (HealthCheck keeps its generated handler).
func (s *MeshWireServer) ServiceDesc() grpc.ServiceDesc {
	v1 := V1_ServiceDesc
	v1.Methods = append([]grpc.MethodDesc(nil), v1.Methods...)
	for i := range v1.Methods {
		if v1.Methods[i].MethodName == "GetRateLimits" {
			v1.Methods[i].Handler = s.getRateLimitsMeshRaw
		}
	}
	return v1
}
