package hipquorum

/*
#include <stdlib.h>
#include "hipquorum.h"
*/
import "C"

import (
	"encoding/binary"
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	pb "github.com/lni/dragonboat/v3/raftpb"
)

// Worker is the quorum side of one step worker (hq_worker_*): it takes every quorum-relevant
// event of the worker's nodes for a step — Peer.Handle's filters, handleLeaderReplicateResp,
// handleLeaderHeartbeatResp, handleLeaderReadIndex, handleCandidateRequestVoteResp,
// handleLeaderCheckQuorum, campaign, appendEntries (execengine.go:923-1000 -> node.go:1113-1157)
// — and returns the step's results. One goroutine per worker, like the step worker itself.
type Worker struct {
	w    *C.hq_worker
	rows *C.hq_step_input  // C memory: the argument blocks of the last step
	strm *C.hq_step_stream
	out  *C.hq_step_output
}

func newWorker(w *C.hq_worker) *Worker {
	x := &Worker{w: w}
	x.rows = (*C.hq_step_input)(C.calloc(1, C.size_t(unsafe.Sizeof(C.hq_step_input{}))))
	x.strm = (*C.hq_step_stream)(C.calloc(1, C.size_t(unsafe.Sizeof(C.hq_step_stream{}))))
	x.out = (*C.hq_step_output)(C.calloc(1, C.size_t(unsafe.Sizeof(C.hq_step_output{}))))
	return x
}

// OpenWorker opens a host worker (decisions on the GPU, bookkeeping on the host).
func OpenWorker(device, nMax int) (*Worker, error) {
	if err := checkABI(); err != nil {
		return nil, err
	}
	var w *C.hq_worker
	if rc := C.hq_worker_open(C.int(device), C.uint32_t(nMax), &w); rc != C.HQ_OK {
		return nil, errors.New(C.GoString(C.hq_last_error(nil)))
	}
	return newWorker(w), nil
}

// OpenDeviceWorker opens a worker whose groups' quorum state is resident in HBM: one GPU thread
// per group takes its events in order, every decision at the event that triggers it
// (hq_dstep_step.hip); commits come back as 4-byte advances when a quarter of the listed groups
// commit, else as one word per listed group or as records; ReadyToReads as 24-byte records
// (EachReady).
func OpenDeviceWorker(device, nMax int) (*Worker, error) {
	if err := checkABI(); err != nil {
		return nil, err
	}
	var w *C.hq_worker
	flags := C.uint32_t(C.HQ_WORKER_ON_DEVICE | C.HQ_WORKER_COMMIT_ADVANCE | C.HQ_WORKER_COMMIT_COLUMN |
		C.HQ_WORKER_READY_COMPACT | C.HQ_WORKER_READY_SLOTS)
	if rc := C.hq_worker_open_ex(C.int(device), C.uint32_t(nMax), flags, &w); rc != C.HQ_OK {
		return nil, errors.New(C.GoString(C.hq_last_error(nil)))
	}
	return newWorker(w), nil
}

func (x *Worker) err(rc C.int) error {
	if rc == C.HQ_OK {
		return nil
	}
	return fmt.Errorf("hipquorum worker error %d: %s", int(rc), C.GoString(C.hq_worker_last_error(x.w)))
}

// Close frees the worker.
// SetWait sets how the worker's goroutine waits for its device step (hq_worker_set_wait:
// C.HQ_WAIT_BLOCK / C.HQ_WAIT_SLEEP / C.HQ_WAIT_SPIN / C.HQ_WAIT_ADAPT, | C.HQ_WAIT_CLOCK).
func (x *Worker) SetWait(mode, pollUs, sleepUs uint32) error {
	return x.err(C.hq_worker_set_wait(x.w, C.uint32_t(mode), C.uint32_t(pollUs), C.uint32_t(sleepUs)))
}

func (x *Worker) Close() {
	C.hq_worker_close(x.w)
	C.free(unsafe.Pointer(x.rows))
	C.free(unsafe.Pointer(x.strm))
	C.free(unsafe.Pointer(x.out))
	x.w = nil
}

// Member is one member of a group as the worker holds it.
type Member = C.hq_member

// GroupState is a group's quorum state (add / set / get).
type GroupState = C.hq_worker_group

// AddGroup registers a group (NodeHost.StartCluster) and returns its handle.
func (x *Worker) AddGroup(g *GroupState, members []Member) (uint32, error) {
	var h C.uint32_t
	var mp *C.hq_member
	if len(members) > 0 {
		mp = &members[0]
	}
	if rc := C.hq_worker_add_group(x.w, g, mp, &h); rc != C.HQ_OK {
		return 0, x.err(rc)
	}
	return uint32(h), nil
}

// SetGroup re-syncs a group after a fallback or a membership change.
func (x *Worker) SetGroup(g *GroupState, members []Member) error {
	var mp *C.hq_member
	if len(members) > 0 {
		mp = &members[0]
	}
	return x.err(C.hq_worker_set_group(x.w, g, mp))
}

// GroupsOutput is the state of the groups listed to GetGroups (hq_groups_output). The arrays live
// in the worker's buffers and are valid until its next GetGroups call; the last step's Output
// stays valid.
type GroupsOutput struct {
	c C.hq_groups_output
}

// GetGroups fetches the state of the listed groups (worker handles, repeats allowed; nil: every
// handle 0 .. n-1 in order) in their state after every earlier step: what the CPU raft needs to
// take over the groups of FallbackClusters or of a ConfigFallback. A device worker gathers one
// packed record per listed group with one small kernel; nothing else of its state crosses the link
// and its readback count does not move.
func (x *Worker) GetGroups(handles []uint32, n int) (*GroupsOutput, error) {
	o := &GroupsOutput{}
	var hp *C.uint32_t
	if handles != nil {
		n = len(handles)
		if n > 0 {
			hp = (*C.uint32_t)(unsafe.Pointer(&handles[0]))
		}
	}
	if rc := C.hq_worker_get_groups(x.w, C.uint64_t(n), hp, &o.c); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return o, nil
}

// Len is the number of listed groups, GPUNanos the HIP-event time of the call (0 on a host worker).
func (o *GroupsOutput) Len() int         { return int(o.c.n_groups) }
func (o *GroupsOutput) GPUNanos() uint64 { return uint64(o.c.gpu_ns) }

// Group returns listed group i: its record, its members in the AddGroup / SetGroup order, and the
// members holding a recorded grant and a recorded rejection (bit j = members[j]).
func (o *GroupsOutput) Group(i int) (g GroupState, members []Member, granted, rejected uint16) {
	n := int(o.c.n_groups)
	g = unsafe.Slice(o.c.groups, n)[i]
	mo := unsafe.Slice((*uint64)(unsafe.Pointer(o.c.member_offsets)), n+1)
	if mo[n] != 0 {
		members = unsafe.Slice(o.c.members, int(mo[n]))[mo[i]:mo[i+1]]
	}
	granted = unsafe.Slice((*uint16)(unsafe.Pointer(o.c.granted)), n)[i]
	rejected = unsafe.Slice((*uint16)(unsafe.Pointer(o.c.rejected)), n)[i]
	return g, members, granted, rejected
}

// Reads returns listed group i's pending ReadIndex queue in queue order, and per entry the members
// that acknowledged its ctx (bit j = members[j]; readStatus.confirmed, readindex.go:21-26).
func (o *GroupsOutput) Reads(i int) (reads []C.hq_read_status, confirmed []uint16) {
	n := int(o.c.n_groups)
	ro := unsafe.Slice((*uint64)(unsafe.Pointer(o.c.read_offsets)), n+1)
	if ro[i] == ro[i+1] {
		return nil, nil
	}
	reads = unsafe.Slice(o.c.reads, int(ro[n]))[ro[i]:ro[i+1]]
	confirmed = unsafe.Slice((*uint16)(unsafe.Pointer(o.c.read_confirmed)), int(ro[n]))[ro[i]:ro[i+1]]
	return reads, confirmed
}

// SetGroups re-syncs the listed groups from the CPU raft, each exactly as SetGroup does (read
// queue and votes cleared, the suspension lifted); members holds the groups' members back to back.
// Every group is validated before any is changed. A device worker writes the groups with one small
// kernel and reads nothing back. Returns the HIP-event time of the call (0 on a host worker).
func (x *Worker) SetGroups(groups []GroupState, members []Member) (uint64, error) {
	if len(groups) == 0 {
		return 0, nil
	}
	var mp *C.hq_member
	if len(members) > 0 {
		mp = &members[0]
	}
	var ns C.uint64_t
	if rc := C.hq_worker_set_groups(x.w, C.uint64_t(len(groups)), &groups[0], mp, &ns); rc != C.HQ_OK {
		return 0, x.err(rc)
	}
	return uint64(ns), nil
}

// StartGroups starts the listed groups on the running worker (NodeHost.StartCluster); members
// holds the groups' members back to back. Every group is validated before any is added: a
// cluster that exists or is listed twice, or any invalid group, fails the call with nothing
// applied. Vacant handles are reused, the most recently vacated first. A device worker writes the
// records with one small kernel and reads nothing back. Returns the groups' handles and the
// HIP-event time of the call (0 on a host worker).
func (x *Worker) StartGroups(groups []GroupState, members []Member) ([]uint32, uint64, error) {
	if len(groups) == 0 {
		return nil, 0, nil
	}
	var mp *C.hq_member
	if len(members) > 0 {
		mp = &members[0]
	}
	handles := make([]uint32, len(groups))
	var ns C.uint64_t
	if rc := C.hq_worker_start_groups(x.w, C.uint64_t(len(groups)), &groups[0], mp,
		(*C.uint32_t)(unsafe.Pointer(&handles[0])), &ns); rc != C.HQ_OK {
		return nil, 0, x.err(rc)
	}
	return handles, uint64(ns), nil
}

// StopGroups stops the listed groups (NodeHost.StopCluster / StopNode): every handle must be live
// and listed once, else nothing is applied. The clusters leave the worker's index and their
// handles become vacant: a later step that lists one gets its events back as deferred. Returns
// the HIP-event time of the call (0 on a host worker).
func (x *Worker) StopGroups(handles []uint32) (uint64, error) {
	if len(handles) == 0 {
		return 0, nil
	}
	var ns C.uint64_t
	if rc := C.hq_worker_stop_groups(x.w, C.uint64_t(len(handles)),
		(*C.uint32_t)(unsafe.Pointer(&handles[0])), &ns); rc != C.HQ_OK {
		return 0, x.err(rc)
	}
	return uint64(ns), nil
}

// PoolInfo is hq_worker_pool_info: the handle space and the member pool of the worker.
type PoolInfo = C.hq_pool_info

// PoolInfo reports the worker's handle space (live and vacant handles), its member pool (records
// held and records of live groups: their difference is what Compact frees) and its lifecycle epoch.
func (x *Worker) PoolInfo() (info PoolInfo, err error) {
	if rc := C.hq_worker_pool_info(x.w, &info); rc != C.HQ_OK {
		return info, x.err(rc)
	}
	return info, nil
}

// Compact closes the member pool's gaps (the ranges of stopped and of relocated groups), between
// steps; handles do not change. Returns the HIP-event time of the call (0 on a host worker or an
// already dense pool).
func (x *Worker) Compact() (uint64, error) {
	var ns C.uint64_t
	if rc := C.hq_worker_compact(x.w, &ns); rc != C.HQ_OK {
		return 0, x.err(rc)
	}
	return uint64(ns), nil
}

// SetTickConfig sets the worker's Raft timer settings (hq_worker_set_tick_config): electionRTT and
// heartbeatRTT are config.ElectionRTT / HeartbeatRTT in ticks, checkQuorum config.CheckQuorum, seed
// the seed of the randomized election timeouts. One config per worker; setting it resets every
// timer.
func (x *Worker) SetTickConfig(electionRTT, heartbeatRTT uint32, checkQuorum bool, seed uint64) error {
	cfg := C.hq_tick_config{election_rtt: C.uint32_t(electionRTT), heartbeat_rtt: C.uint32_t(heartbeatRTT),
		seed: C.uint64_t(seed)}
	if checkQuorum {
		cfg.check_quorum = 1
	}
	if rc := C.hq_worker_set_tick_config(x.w, &cfg); rc != C.HQ_OK {
		return x.err(rc)
	}
	return nil
}

// TickOutput is what is due after one tick (hq_worker_tick): three lists of worker handles in
// ascending order, in the worker's buffers (pinned host memory on a device worker) and valid until
// its next Tick.
type TickOutput struct {
	c C.hq_tick_output
}

func tickList(p *C.uint32_t, n C.uint64_t) []uint32 {
	if n == 0 {
		return nil
	}
	return unsafe.Slice((*uint32)(unsafe.Pointer(p)), int(n))
}

// CheckQuorum lists the leaders whose step carries HQ_EV_CHECK_QUORUM, Election the followers and
// candidates whose step carries HQ_EV_ELECTION (the caller still filters hasConfigChangeToApply),
// Heartbeat the leaders to pass to Heartbeats / HeartbeatBatches after that step.
func (o *TickOutput) CheckQuorum() []uint32 { return tickList(o.c.check_quorum, o.c.n_check_quorum) }
func (o *TickOutput) Heartbeat() []uint32   { return tickList(o.c.heartbeat, o.c.n_heartbeat) }
func (o *TickOutput) Election() []uint32    { return tickList(o.c.election, o.c.n_election) }

// Ticked is the number of groups advanced, GPUNanos the HIP-event time of the call's kernels (0 on
// a host worker).
func (o *TickOutput) Ticked() uint64   { return uint64(o.c.n_ticked) }
func (o *TickOutput) GPUNanos() uint64 { return uint64(o.c.gpu_ns) }

// Tick advances every live, unsuspended group by one tick (raft.tick, raft.go:525-636), once per
// LocalTick. contact lists the handles of the followers that heard from their leader since the
// last Tick (leaderIsAvailable, raft.go:1859-1861; repeats allowed). The caller's order within a
// tick interval: Tick, then the step with the CheckQuorum / Election events of the listed handles,
// then Heartbeats over Heartbeat(). A device worker ticks its resident state with three small
// kernels: nothing of the state is read back.
func (x *Worker) Tick(contact []uint32) (*TickOutput, error) {
	var cp *C.uint32_t
	if len(contact) > 0 {
		cp = (*C.uint32_t)(unsafe.Pointer(&contact[0]))
	}
	o := &TickOutput{}
	if rc := C.hq_worker_tick(x.w, C.uint64_t(len(contact)), cp, &o.c); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return o, nil
}

// Timer is hq_timer: a group's electionTick, heartbeatTick and randomizedElectionTimeout.
type Timer = C.hq_timer

// TickTimeout is the randomized election timeout, in [electionRTT, 2 electionRTT), the worker draws
// for a group at (term, state) under seed (hq_tick_timeout).
func TickTimeout(seed, clusterID, term uint64, state, electionRTT uint32) uint32 {
	return uint32(C.hq_tick_timeout(C.uint64_t(seed), C.uint64_t(clusterID), C.uint64_t(term),
		C.uint32_t(state), C.uint32_t(electionRTT)))
}

// GetTimers fetches the timers of the listed handles (repeats allowed), what the CPU raft takes
// over with a suspended group; a timer with a pending reset comes as reset.
func (x *Worker) GetTimers(handles []uint32) ([]Timer, error) {
	if len(handles) == 0 {
		return nil, nil
	}
	out := make([]Timer, len(handles))
	if rc := C.hq_worker_get_timers(x.w, C.uint64_t(len(handles)),
		(*C.uint32_t)(unsafe.Pointer(&handles[0])), &out[0]); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return out, nil
}

// SetTimers hands the listed handles (each once) back with their counters, after SetGroups: the
// counters continue under the group's current term and state; a randomized_timeout of 0 is drawn
// by the worker. Every entry is validated before any is applied.
func (x *Worker) SetTimers(handles []uint32, timers []Timer) error {
	if len(handles) == 0 {
		return nil
	}
	if len(timers) != len(handles) {
		return fmt.Errorf("hipquorum: %d timers for %d handles", len(timers), len(handles))
	}
	if rc := C.hq_worker_set_timers(x.w, C.uint64_t(len(handles)),
		(*C.uint32_t)(unsafe.Pointer(&handles[0])), &timers[0]); rc != C.HQ_OK {
		return x.err(rc)
	}
	return nil
}

// ReceivedHeartbeat is hq_hb_received: the fields of a received Heartbeat (type 17) the follower
// path reads. HeartbeatReply is hq_hb_reply (one per message: type 0, HQ_MSG_HEARTBEAT_RESP or
// HQ_MSG_NOOP), HeartbeatResult hq_hb_group_result (one per listed group), WireMessage
// hq_wire_message.
type ReceivedHeartbeat = C.hq_hb_received
type HeartbeatReply = C.hq_hb_reply
type HeartbeatResult = C.hq_hb_group_result
type WireMessage = C.hq_wire_message

// ReceivedOutput is what a step interval's received Heartbeats did (hq_worker_heartbeats_received):
// the replies at their messages' indexes and the per-group results in input order, in the
// worker's buffers (pinned host memory on a device worker), valid until its next
// HeartbeatsReceived.
type ReceivedOutput struct {
	c C.hq_hb_received_output
}

func (o *ReceivedOutput) Replies() []HeartbeatReply {
	if o.c.n_msgs == 0 {
		return nil
	}
	return unsafe.Slice((*HeartbeatReply)(unsafe.Pointer(o.c.replies)), int(o.c.n_msgs))
}

func (o *ReceivedOutput) Results() []HeartbeatResult {
	if o.c.n_groups == 0 {
		return nil
	}
	return unsafe.Slice((*HeartbeatResult)(unsafe.Pointer(o.c.results)), int(o.c.n_groups))
}

// Resps and NoOPs count the replies by type; Contacts, Committed, StateChanged and Suspended the
// groups with HQ_HBR_CONTACT, HQ_HBR_COMMITTED, a becomeFollower and HQ_HBR_SUSPENDED.
func (o *ReceivedOutput) Resps() uint64        { return uint64(o.c.n_resp) }
func (o *ReceivedOutput) NoOPs() uint64        { return uint64(o.c.n_noop) }
func (o *ReceivedOutput) Contacts() uint64     { return uint64(o.c.n_contact) }
func (o *ReceivedOutput) Committed() uint64    { return uint64(o.c.n_committed) }
func (o *ReceivedOutput) StateChanged() uint64 { return uint64(o.c.n_state_changed) }
func (o *ReceivedOutput) Suspended() uint64    { return uint64(o.c.n_suspended) }
func (o *ReceivedOutput) GPUNanos() uint64     { return uint64(o.c.gpu_ns) }

// HeartbeatsReceived handles the Heartbeats that lead the queues of the listed groups (each handle
// at most once; group i's messages are msgs[offsets[i]:offsets[i+1]] in arrival order) where the
// state lives, as Peer.Handle would (raft.go:1416-1452, 1869-1873, 1963-1966, 1302-1310), before
// the interval's step. The groups that heard from their leader are marked for the next Tick inside
// the worker: its contact list carries only what Replicate caused. The caller applies commitTo
// from the results' commit column to its own log and sends the replies (ExpandHeartbeatReplies).
// A group whose result carries HQ_HBR_SUSPENDED handled nothing: its messages go to the CPU raft.
func (x *Worker) HeartbeatsReceived(groups []uint32, offsets []uint64, msgs []ReceivedHeartbeat,
	checkQuorum bool) (*ReceivedOutput, error) {
	if len(offsets) != len(groups)+1 {
		return nil, fmt.Errorf("hipquorum: %d offsets for %d groups", len(offsets), len(groups))
	}
	in := C.hq_hb_received_input{n_groups: C.uint64_t(len(groups)),
		offsets: (*C.uint64_t)(unsafe.Pointer(&offsets[0]))}
	if len(groups) > 0 {
		in.groups = (*C.uint32_t)(unsafe.Pointer(&groups[0]))
	}
	if len(msgs) > 0 {
		in.msgs = &msgs[0]
	}
	if checkQuorum {
		in.check_quorum = 1
	}
	o := &ReceivedOutput{}
	if rc := C.hq_worker_heartbeats_received(x.w, &in, &o.c); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return o, nil
}

// ExpandHeartbeatReplies writes the replies of o (the output of HeartbeatsReceived over the same
// groups, offsets and msgs) with a type as wire messages for the batch encoder, in input order;
// clusterIDs and nodeIDs are per listed group. Stateless (hq_heartbeat_replies_expand).
func ExpandHeartbeatReplies(groups []uint32, offsets []uint64, msgs []ReceivedHeartbeat, o *ReceivedOutput,
	clusterIDs, nodeIDs []uint64) ([]WireMessage, error) {
	if len(offsets) != len(groups)+1 || len(clusterIDs) != len(groups) || len(nodeIDs) != len(groups) {
		return nil, fmt.Errorf("hipquorum: columns do not match %d groups", len(groups))
	}
	if len(groups) == 0 || len(msgs) == 0 {
		return nil, nil
	}
	in := C.hq_hb_received_input{n_groups: C.uint64_t(len(groups)),
		groups: (*C.uint32_t)(unsafe.Pointer(&groups[0])), offsets: (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		msgs: &msgs[0]}
	out := make([]WireMessage, len(msgs))
	var n C.uint64_t
	if rc := C.hq_heartbeat_replies_expand(&in, &o.c, (*C.uint64_t)(unsafe.Pointer(&clusterIDs[0])),
		(*C.uint64_t)(unsafe.Pointer(&nodeIDs[0])), &out[0], C.uint64_t(len(out)), &n); rc != C.HQ_OK {
		return nil, fmt.Errorf("hipquorum: hq_heartbeat_replies_expand: %d", int(rc))
	}
	return out[:n], nil
}

// Output is one step's results; the lists live in the worker's pinned buffers and are valid
// until the worker's next step.
type Output struct {
	c      *C.hq_step_output
	listed int
}

// Step hands over the step's events as rows: groups[i]'s events are
// events[offsets[i]:offsets[i+1]] (local ReadIndex, received messages, tick messages, proposals —
// node.handleEvents order). All three slices must be views of pinned C memory.
func (x *Worker) Step(groups []uint32, offsets []uint64, events []C.hq_event) (*Output, error) {
	*x.rows = C.hq_step_input{
		n_groups: C.uint64_t(len(groups)),
		groups:   (*C.uint32_t)(unsafe.Pointer(&groups[0])),
		offsets:  (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		events:   (*C.hq_event)(unsafe.Pointer(&events[0])),
	}
	if rc := C.hq_worker_step(x.w, x.rows, x.out); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return &Output{c: x.out, listed: len(groups)}, nil
}

// StreamBuf is one step's input as an event stream in pinned C memory: per event a header byte
// and the LEB128 varints of the fields its handler reads (include/hipquorum.h "event streams"),
// per node one 2-byte byte count (hq_step_stream.sizes16, the bytes-only sized form: the engine
// counts the events from the bytes).
type StreamBuf struct {
	Groups  []uint32 // worker handles, or nil: every handle 0 .. len(Sizes)-1 in order
	Sizes   []uint16 // per node its byte count (hq_step_stream.sizes16: the engine counts events)
	NEvents uint64
	Bytes   []byte // a pinned region; len = bytes written so far
	start   int
	events  int
	prev    prevMsg
}

// the node's stream state the header codes refer back to: its previous message term, its
// previous ReplicateResp's index (code 4), its previous HeartbeatResp's ctx (code 5)
type prevMsg struct {
	term, index, hint, high uint64
	haveIndex               bool
}

// BeginNode starts a node's run of events.
func (b *StreamBuf) BeginNode() {
	b.start = len(b.Bytes)
	b.events = 0
	b.prev = prevMsg{}
}

// EndNode closes the node's run with its size word.
func (b *StreamBuf) EndNode(handle uint32) {
	if b.Groups != nil {
		b.Groups = append(b.Groups, handle)
	}
	b.Sizes = append(b.Sizes, uint16(len(b.Bytes)-b.start))
	b.NEvents += uint64(b.events)
}

func (b *StreamBuf) header(code uint32, reject bool, term uint64) {
	h := byte(C.HQ_EV_MESSAGE) | byte(code<<3)
	if reject {
		h |= 0x40
	}
	same := term == b.prev.term
	if same {
		h |= 0x80
	}
	b.Bytes = append(b.Bytes, h)
	b.prev.term = term
	b.events++
}

// AppendReplicateResp encodes a ReplicateResp (code 0, or code 4 without the index when it
// repeats the node's previous ReplicateResp in this step).
func (b *StreamBuf) AppendReplicateResp(from, term, index uint64, reject bool) {
	code := uint32(0)
	if b.prev.haveIndex && index == b.prev.index {
		code = 4
	}
	b.prev.index, b.prev.haveIndex = index, true
	same := term == b.prev.term
	b.header(code, reject, term)
	b.Bytes = binary.AppendUvarint(b.Bytes, from)
	if !same {
		b.Bytes = binary.AppendUvarint(b.Bytes, term)
	}
	if code == 0 {
		b.Bytes = binary.AppendUvarint(b.Bytes, index)
	}
}

// AppendHeartbeatResp encodes a HeartbeatResp (code 2, or code 5 without the ctx when it repeats
// the node's previous HeartbeatResp ctx; 0 / 0 before the first).
func (b *StreamBuf) AppendHeartbeatResp(from, term uint64, ctx pb.SystemCtx) {
	code := uint32(2)
	if ctx.Low == b.prev.hint && ctx.High == b.prev.high {
		code = 5
	}
	b.prev.hint, b.prev.high = ctx.Low, ctx.High
	same := term == b.prev.term
	b.header(code, false, term)
	b.Bytes = binary.AppendUvarint(b.Bytes, from)
	if !same {
		b.Bytes = binary.AppendUvarint(b.Bytes, term)
	}
	if code == 2 {
		b.Bytes = binary.AppendUvarint(b.Bytes, ctx.Low)
		b.Bytes = binary.AppendUvarint(b.Bytes, ctx.High)
	}
}

// AppendPropose encodes a proposal of n entries (handleLeaderPropose).
func (b *StreamBuf) AppendPropose(n uint64) {
	b.Bytes = append(b.Bytes, byte(C.HQ_EV_PROPOSE))
	b.Bytes = binary.AppendUvarint(b.Bytes, n)
	b.events++
}

// AppendLocalRead encodes the node's own ReadIndex (Peer.ReadIndex, node.go:1197).
func (b *StreamBuf) AppendLocalRead(ctx pb.SystemCtx) {
	b.Bytes = append(b.Bytes, byte(C.HQ_EV_READ))
	b.Bytes = binary.AppendUvarint(b.Bytes, ctx.Low)
	b.Bytes = binary.AppendUvarint(b.Bytes, ctx.High)
	b.events++
}

func (x *Worker) setStream(b *StreamBuf) {
	*x.strm = C.hq_step_stream{
		n_groups: C.uint64_t(len(b.Sizes)),
		bytes:    (*C.uint8_t)(unsafe.Pointer(&b.Bytes[0])),
		sizes16:  (*C.uint16_t)(unsafe.Pointer(&b.Sizes[0])),
		n_events: C.uint64_t(b.NEvents),
		n_bytes:  C.uint64_t(len(b.Bytes)),
	}
	if b.Groups != nil {
		x.strm.groups = (*C.uint32_t)(unsafe.Pointer(&b.Groups[0]))
	}
}

// StepStream steps the worker over an event stream (Bytes, Sizes and Groups in pinned memory).
func (x *Worker) StepStream(b *StreamBuf) (*Output, error) {
	x.setStream(b)
	if rc := C.hq_worker_step_stream(x.w, x.strm, x.out); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return &Output{c: x.out, listed: len(b.Sizes)}, nil
}

// StepJobs steps several device workers of one GPU at once through shared launches (the 16
// step-worker goroutines each calling their own worker, execengine.go:923-1000).
func StepJobs(ws []*Worker, bufs []*StreamBuf) ([]*Output, error) {
	n := len(ws)
	if n == 0 || n != len(bufs) {
		return nil, errors.New("hipquorum: one stream per worker")
	}
	mem := C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.hq_step_job{})))
	defer C.free(mem)
	jobs := unsafe.Slice((*C.hq_step_job)(mem), n)
	for i, w := range ws {
		w.setStream(bufs[i])
		jobs[i] = C.hq_step_job{worker: w.w, stream: w.strm, out: w.out}
	}
	rc := C.hq_worker_step_jobs(&jobs[0], C.uint32_t(n))
	outs := make([]*Output, n)
	for i, w := range ws {
		if jobs[i].rc != C.HQ_OK {
			return nil, w.err(jobs[i].rc)
		}
		outs[i] = &Output{c: w.out, listed: len(bufs[i].Sizes)}
	}
	if rc != C.HQ_OK {
		return nil, fmt.Errorf("hq_worker_step_jobs: %d", int(rc))
	}
	return outs, nil
}

// EachCommit calls fn(listed index, new committed index) for every group that committed in the
// step, whichever form the step returned: the advance column (added to the committed index the
// node holds: committedOf), the index column, or the (cluster, index) records (listedOf maps a
// cluster id to its listed index). The node then applies commitTo (logentry.go:323-332).
func (o *Output) EachCommit(committedOf func(i int) uint64, listedOf func(clusterID uint64) int,
	fn func(i int, committed uint64)) {
	switch {
	case o.c.committed_advance != nil:
		adv := unsafe.Slice((*uint32)(unsafe.Pointer(o.c.committed_advance)), o.listed)
		for i, a := range adv {
			if a != 0 {
				fn(i, committedOf(i)+uint64(a))
			}
		}
	case o.c.committed_column != nil:
		col := unsafe.Slice((*uint64)(unsafe.Pointer(o.c.committed_column)), o.listed)
		for i, c := range col {
			if c != 0 {
				fn(i, c)
			}
		}
	default:
		if o.c.n_commits == 0 {
			return
		}
		recs := unsafe.Slice(o.c.commits, int(o.c.n_commits))
		for _, r := range recs {
			fn(listedOf(uint64(r.cluster_id)), uint64(r.committed))
		}
	}
}

// ReadyToRead lists the step's released reads (pb.ReadyToRead, raftpb/raft.go:54-57) when the
// step returned them as full records (nil when they are compact: EachReady reads both).
func (o *Output) ReadyToRead() []C.hq_ready_to_read {
	if o.c.n_ready == 0 || o.c.ready == nil {
		return nil
	}
	return unsafe.Slice(o.c.ready, int(o.c.n_ready))
}

// EachReady calls fn(listed index, pb.ReadyToRead) for every released read of the step, in the
// reference's order (listed order), whichever form the step returned: the per-tile slots
// (HQ_WORKER_READY_SLOTS) and the list — 24-byte records (HQ_WORKER_READY_COMPACT: the index is
// the group's committed index before the step, committedBefore, plus the record's delta) or full
// records (listedOf maps a cluster id to its listed index) — merged by listed index (a group's
// reads are all in one of the two). The node then calls processReadyToRead (node.go:1026-1031).
func (o *Output) EachReady(committedBefore func(i int) uint64, listedOf func(clusterID uint64) int,
	fn func(i int, r pb.ReadyToRead)) {
	compact := func(r C.hq_ready_compact) (int, pb.ReadyToRead) {
		i := int(r.pos)
		return i, pb.ReadyToRead{Index: committedBefore(i) + uint64(int64(r.delta)),
			SystemCtx: pb.SystemCtx{Low: uint64(r.ctx_low), High: uint64(r.ctx_high)}}
	}
	// the list, one record at a time with its listed index
	k, n := 0, int(o.c.n_ready)
	listAt := func(k int) (int, pb.ReadyToRead) {
		if o.c.ready_compact != nil {
			return compact(unsafe.Slice(o.c.ready_compact, n)[k])
		}
		var f C.hq_ready_to_read = unsafe.Slice(o.c.ready, n)[k]
		return listedOf(uint64(f.cluster_id)), pb.ReadyToRead{Index: uint64(f.index),
			SystemCtx: pb.SystemCtx{Low: uint64(f.ctx_low), High: uint64(f.ctx_high)}}
	}
	if o.c.ready_slots != nil {
		tiles := int(o.c.n_ready_tiles)
		counts := unsafe.Slice((*uint32)(unsafe.Pointer(o.c.ready_slot_counts)), tiles)
		slots := unsafe.Slice(o.c.ready_slots, tiles*256)
		for t, c := range counts {
			for _, r := range slots[t*256 : t*256+int(c)] {
				i, rr := compact(r)
				for ; k < n; k++ { // the list's reads of the groups before this one
					j, lr := listAt(k)
					if j > i {
						break
					}
					fn(j, lr)
				}
				fn(i, rr)
			}
		}
	}
	for ; k < n; k++ {
		fn(listAt(k))
	}
}

// HeartbeatOutput is what the leaders among the listed groups send on a LeaderHeartbeat tick
// (hq_worker_heartbeats: broadcastHeartbeatMessage, raft.go:812-848, sent from :1577-1579 with
// readIndex.peepCtx, readindex.go:69-75), compact: one word per listed group, a record per member
// that is behind the committed index, a record per group whose heartbeats carry a ctx. The arrays
// live in the worker's buffers and are valid until its next Heartbeats call; the last step's
// Output stays valid across the call.
type HeartbeatOutput struct {
	c C.hq_heartbeat_output
}

// Heartbeats computes the heartbeats of the listed groups (worker handles, repeats allowed; nil:
// every handle 0 .. n-1 in order) in their state after every earlier step. It runs on the
// heartbeat tick, and after a step for the groups that accepted a ReadIndex
// (handleLeaderReadIndex broadcasts with the new ctx, which is then peepCtx). A device worker
// reads its resident state with two small kernels; nothing of the state comes back but the
// output.
func (x *Worker) Heartbeats(groups []uint32, n int) (*HeartbeatOutput, error) {
	o := &HeartbeatOutput{}
	var gp *C.uint32_t
	if groups != nil {
		n = len(groups)
		if n > 0 {
			gp = (*C.uint32_t)(unsafe.Pointer(&groups[0]))
		}
	}
	if rc := C.hq_worker_heartbeats(x.w, C.uint64_t(n), gp, &o.c); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return o, nil
}

// Messages is the number of Heartbeat messages the output stands for.
func (o *HeartbeatOutput) Messages() uint64 { return uint64(o.c.n_messages) }

// GPUNanos is the HIP-event time of the call's kernels (0 on a host worker).
func (o *HeartbeatOutput) GPUNanos() uint64 { return uint64(o.c.gpu_ns) }

// Each calls fn for every Heartbeat to send, in listed order, then member order: pos is the
// group's place in the list and member the destination's place in the group's member list (its
// AddGroup / SetGroup order). With commitIsMatch the message's Commit is match (the member is
// behind, sendHeartbeatMessage's min(match, committed), raft.go:812-822); otherwise it is the
// group's committed index, which the node holds. Term is the node's term
// (finalizeMessageTerm, raft.go:650-652); Hint / HintHigh come from EachCtx.
func (o *HeartbeatOutput) Each(fn func(pos int, member int, commitIsMatch bool, match uint64)) {
	n := int(o.c.n_groups)
	if n == 0 {
		return
	}
	words := unsafe.Slice((*uint32)(unsafe.Pointer(o.c.words)), n)
	var lags []C.hq_heartbeat_lag
	if o.c.n_lags != 0 {
		lags = unsafe.Slice(o.c.lags, int(o.c.n_lags))
	}
	k := 0
	for pos, w := range words {
		for m := 0; m < 16 && w&0xFFFF>>uint(m) != 0; m++ {
			if w>>uint(m)&1 == 0 {
				continue
			}
			if w>>uint(16+m)&1 != 0 {
				var l C.hq_heartbeat_lag = lags[k]
				k++
				fn(pos, m, true, uint64(l.match))
			} else {
				fn(pos, m, false, 0)
			}
		}
	}
}

// EachCtx calls fn(pos, ctx) for every listed group whose heartbeats carry a ReadIndex ctx (the
// last pending read's, readindex.go:69-75), in listed order; every other group's carry the zero
// ctx.
func (o *HeartbeatOutput) EachCtx(fn func(pos int, ctx pb.SystemCtx)) {
	if o.c.n_ctxs == 0 {
		return
	}
	for _, r := range unsafe.Slice(o.c.ctxs, int(o.c.n_ctxs)) {
		var c C.hq_heartbeat_ctx = r
		fn(int(c.pos), pb.SystemCtx{Low: uint64(c.ctx_low), High: uint64(c.ctx_high)})
	}
}

// RouteNone is HQ_ROUTE_NONE: the member has no destination and its heartbeat is not marshalled.
const RouteNone = uint16(0xFFFF)

// SetHeartbeatRoutes tells the worker where the members of groups [firstHandle, firstHandle +
// len(routes)/16) live: 16 words per group, word i the destination index of member i of the
// group's member list (its AddGroup / SetGroup order), RouteNone for none. The worker keeps the
// routes until they are set again; a device worker uploads them with the next HeartbeatBatches.
func (x *Worker) SetHeartbeatRoutes(firstHandle uint32, routes []uint16) error {
	if len(routes)%16 != 0 {
		return fmt.Errorf("hipquorum: SetHeartbeatRoutes: %d route words, not 16 per group", len(routes))
	}
	if len(routes) == 0 {
		return nil
	}
	rc := C.hq_worker_set_heartbeat_routes(x.w, C.uint32_t(firstHandle), C.uint64_t(len(routes)/16),
		(*C.uint16_t)(unsafe.Pointer(&routes[0])))
	if rc != C.HQ_OK {
		return x.err(rc)
	}
	return nil
}

// HeartbeatBatch is one marshalled MessageBatch of a HeartbeatBatches call: Bytes is a view of the
// worker's buffer (pinned host memory on a device worker), not a copy, ready for the transport to
// send to destination Dest as it is.
type HeartbeatBatch struct {
	Dest     uint32
	Messages uint32
	Bytes    []byte
}

// HeartbeatBatchOutput is the result of HeartbeatBatches. The batches are ordered by destination,
// then in sequence, and are valid until the worker's next HeartbeatBatches call or Close.
type HeartbeatBatchOutput struct {
	c       C.hq_heartbeat_batches
	Batches []HeartbeatBatch
}

// Messages is the number of Heartbeat messages marshalled, Unrouted the number left out because
// their member's route is RouteNone, Bytes the size of all batches, GPUNanos the HIP-event time of
// the call's kernels (0 on a host worker).
func (o *HeartbeatBatchOutput) Messages() uint64 { return uint64(o.c.n_messages) }
func (o *HeartbeatBatchOutput) Unrouted() uint64 { return uint64(o.c.n_unrouted) }
func (o *HeartbeatBatchOutput) Bytes() uint64    { return uint64(o.c.n_bytes) }
func (o *HeartbeatBatchOutput) GPUNanos() uint64 { return uint64(o.c.gpu_ns) }

// HeartbeatBatches marshals the heartbeats of the listed groups (as Heartbeats lists them) into
// complete MessageBatch byte strings, one run of batches per destination of SetHeartbeatRoutes
// (hq_worker_heartbeat_batches). deploymentID and source are the batch's DeploymentId and
// SourceAddress; nDest is the number of destinations; a batch is cut after every batchMessages
// messages (0: one batch per destination), which the caller chooses so that 113 * batchMessages
// plus the trailer stays under its batch limit (settings.MaxMessageBatchSize,
// transport.go:460-472). A device worker writes the bytes on the GPU; the host touches no message.
func (x *Worker) HeartbeatBatches(groups []uint32, n int, deploymentID uint64, source string,
	nDest uint32, batchMessages uint32) (*HeartbeatBatchOutput, error) {
	o := &HeartbeatBatchOutput{}
	var gp *C.uint32_t
	if groups != nil {
		n = len(groups)
		if n > 0 {
			gp = (*C.uint32_t)(unsafe.Pointer(&groups[0]))
		}
	}
	src := []byte(source)
	var cfg C.hq_heartbeat_wire_config
	cfg.deployment_id = C.uint64_t(deploymentID)
	cfg.n_dest = C.uint32_t(nDest)
	cfg.batch_messages = C.uint32_t(batchMessages)
	cfg.source_len = C.uint32_t(len(src))
	if len(src) > 0 {
		// (C memory: the struct passed to C may not hold a Go pointer)
		cfg.source = (*C.uint8_t)(C.CBytes(src))
		defer C.free(unsafe.Pointer(cfg.source))
	}
	if rc := C.hq_worker_heartbeat_batches(x.w, C.uint64_t(n), gp, &cfg, &o.c); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	if o.c.n_batches == 0 {
		return o, nil
	}
	all := unsafe.Slice((*byte)(unsafe.Pointer(o.c.bytes)), int(o.c.n_bytes))
	table := unsafe.Slice(o.c.batches, int(o.c.n_batches))
	o.Batches = make([]HeartbeatBatch, len(table))
	for i := range table {
		var b C.hq_heartbeat_batch = table[i]
		o.Batches[i] = HeartbeatBatch{Dest: uint32(b.dest), Messages: uint32(b.n_messages),
			Bytes: all[b.offset : b.offset+b.len : b.offset+b.len]}
	}
	return o, nil
}

// ConfigChange is one membership change of ApplyConfigChanges: Group is the worker's handle of the
// cluster, Type the pb.ConfigChangeType (AddNode 0, RemoveNode 1, AddObserver 2, AddWitness 3).
type ConfigChange struct {
	Group  uint32
	Type   pb.ConfigChangeType
	NodeID uint64
}

// ConfigChangeOutput is the result of ApplyConfigChanges. The arrays live in the worker's buffers
// and are valid until its next ApplyConfigChanges call; the last step's Output stays valid.
type ConfigChangeOutput struct {
	c C.hq_config_output
	n int
}

// Config-change statuses (HQ_CC_*): Fallback means nothing was applied and the group is suspended
// until SetGroup re-syncs it from the CPU raft; Suspended that it was suspended already.
const (
	ConfigApplied   = uint32(C.HQ_CC_APPLIED)
	ConfigNoop      = uint32(C.HQ_CC_NOOP)
	ConfigFallback  = uint32(C.HQ_CC_FALLBACK)
	ConfigSuspended = uint32(C.HQ_CC_SUSPENDED)
)

// ApplyConfigChanges applies membership changes to the worker's quorum state
// (hq_worker_config_changes: handleNodeConfigChange, raft.go:1540-1559, with removeNode's
// tryCommit, raft.go:1194-1198), each group at most once. It is called between steps, where
// node.ApplyConfigChange holds raftMu (node.go:229-251). A device worker edits its resident member
// records with one small kernel: nothing of the state is read back.
func (x *Worker) ApplyConfigChanges(changes []ConfigChange) (*ConfigChangeOutput, error) {
	o := &ConfigChangeOutput{n: len(changes)}
	cs := make([]C.hq_config_change, len(changes))
	for i, ch := range changes {
		cs[i] = C.hq_config_change{group: C.uint32_t(ch.Group), _type: C.uint32_t(ch.Type),
			node_id: C.uint64_t(ch.NodeID)}
	}
	var cp *C.hq_config_change
	if len(cs) > 0 {
		cp = &cs[0]
	}
	if rc := C.hq_worker_config_changes(x.w, C.uint64_t(len(cs)), cp, &o.c); rc != C.HQ_OK {
		return nil, x.err(rc)
	}
	return o, nil
}

// Status lists one status per change, in input order.
func (o *ConfigChangeOutput) Status() []uint32 {
	if o.n == 0 {
		return nil
	}
	return unsafe.Slice((*uint32)(unsafe.Pointer(o.c.status)), o.n)
}

// Commits lists the groups whose committed index a removal advanced (the caller then broadcasts
// Replicate for them, raft.go:1195-1197), in input order.
func (o *ConfigChangeOutput) Commits() []C.hq_commit_event {
	if o.c.n_commits == 0 {
		return nil
	}
	return unsafe.Slice((*C.hq_commit_event)(unsafe.Pointer(o.c.commits)), int(o.c.n_commits))
}

// Fallbacks is the number of groups the call suspended, GPUNanos the HIP-event time of the call
// (0 on a host worker).
func (o *ConfigChangeOutput) Fallbacks() uint64 { return uint64(o.c.n_fallback) }
func (o *ConfigChangeOutput) GPUNanos() uint64  { return uint64(o.c.gpu_ns) }

// StateChanges lists the step's leader / follower / candidate transitions.
func (o *Output) StateChanges() []C.hq_state_change {
	if o.c.n_state_changes == 0 {
		return nil
	}
	return unsafe.Slice(o.c.state_changes, int(o.c.n_state_changes))
}

// FallbackClusters lists the clusters whose later events go through the CPU raft this step.
func (o *Output) FallbackClusters() []uint64 {
	if o.c.n_fallback_groups == 0 {
		return nil
	}
	return unsafe.Slice((*uint64)(unsafe.Pointer(o.c.fallback_groups)), int(o.c.n_fallback_groups))
}

// Msg16 packs one received message for the library's encoder (include/hipquorum.h "Compact
// messages"). A field that does not fit (a node id >= 2^16, a term >= 2^32, a HeartbeatResp ctx
// with a high word that is not the node's own pending read) needs the escape (HQ_EV16_FULL and
// the 56-byte row in 4 records); ok is false then.
func Msg16(m *pb.Message, readCtx pb.SystemCtx) (r C.hq_event16, ok bool) {
	if m.From >= 1<<16 || m.Term >= 1<<32 || uint64(m.Type) >= 256 {
		return r, false
	}
	r = C.hq_event16{kind: C.uint8_t(C.HQ_EV_MESSAGE), _type: C.uint8_t(m.Type),
		from: C.uint16_t(m.From), term: C.uint32_t(m.Term)}
	if m.Reject {
		r.kind |= 8
	}
	switch m.Type {
	case pb.HeartbeatResp, pb.ReadIndex:
		if m.Hint == readCtx.Low && m.HintHigh == readCtx.High && m.Hint|m.HintHigh != 0 {
			r.kind |= C.HQ_EV16_READ_CTX
		} else if m.HintHigh != 0 {
			return r, false
		} else {
			r.value = C.uint64_t(m.Hint)
		}
	default:
		r.value = C.uint64_t(m.LogIndex)
	}
	return r, true
}

// Encode16 encodes a step's compact records (recs[offsets[i]:offsets[i+1]] for listed node i)
// into the stream buffer's bytes and size words on `threads` native threads.
func Encode16(offsets []uint64, recs []C.hq_event16, b *StreamBuf, threads int) error {
	nGroups := len(offsets) - 1
	var nEvents, nBytes C.uint64_t
	var rp *C.hq_event16
	if len(recs) > 0 {
		rp = &recs[0]
	}
	rc := C.hq_events16_encode_sized(C.uint64_t(nGroups), (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		rp, (*C.uint8_t)(unsafe.Pointer(&b.Bytes[:cap(b.Bytes)][0])), C.uint64_t(cap(b.Bytes)),
		(*C.uint32_t)(unsafe.Pointer(&b.Sizes[:cap(b.Sizes)][0])), &nEvents, &nBytes, C.uint32_t(threads))
	if rc != C.HQ_OK {
		return fmt.Errorf("hq_events16_encode_sized: %d", int(rc))
	}
	b.Bytes = b.Bytes[:int(nBytes)]
	b.Sizes = b.Sizes[:nGroups]
	b.NEvents = uint64(nEvents)
	return nil
}

// Encode16Job is one step worker's step for EncodeMany: its compact records and stream buffer.
type Encode16Job struct {
	Offsets []uint64
	Recs    []C.hq_event16
	Buf     *StreamBuf
}

// EncodeMany encodes the steps of several step workers in one call whose `threads` native
// threads split the records of all of them evenly (hq_events16_encode_sized_multi); each
// buffer ends as its own Encode16 would leave it. The Go slices the C array points at are
// pinned for the call (cgo: Go pointers stored in C memory must be pinned).
func EncodeMany(jobs []Encode16Job, threads int) error {
	if len(jobs) == 0 {
		return nil
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	mem := C.malloc(C.size_t(len(jobs)) * C.size_t(unsafe.Sizeof(C.hq_encode16_job{})))
	defer C.free(mem)
	cj := unsafe.Slice((*C.hq_encode16_job)(mem), len(jobs))
	for i, j := range jobs {
		b := j.Buf
		pin.Pin(&j.Offsets[0])
		bytes := b.Bytes[:cap(b.Bytes)]
		sizes := b.Sizes[:cap(b.Sizes)]
		pin.Pin(&bytes[0])
		pin.Pin(&sizes[0])
		cj[i] = C.hq_encode16_job{n_groups: C.uint64_t(len(j.Offsets) - 1),
			offsets16: (*C.uint64_t)(unsafe.Pointer(&j.Offsets[0])),
			out:       (*C.uint8_t)(unsafe.Pointer(&bytes[0])), cap: C.uint64_t(len(bytes)),
			sizes16: (*C.uint16_t)(unsafe.Pointer(&sizes[0]))}
		if len(j.Recs) > 0 {
			pin.Pin(&j.Recs[0])
			cj[i].recs = &j.Recs[0]
		}
	}
	rc := C.hq_events16_encode_sized_multi(&cj[0], C.uint32_t(len(jobs)), C.uint32_t(threads))
	for i, j := range jobs {
		if cj[i].rc != C.HQ_OK {
			return fmt.Errorf("hq_events16_encode_sized_multi: job %d: %d", i, int(cj[i].rc))
		}
		j.Buf.Bytes = j.Buf.Bytes[:int(cj[i].n_bytes)]
		j.Buf.Sizes = j.Buf.Sizes[:len(j.Offsets)-1]
		j.Buf.NEvents = uint64(cj[i].n_events)
	}
	if rc != C.HQ_OK {
		return fmt.Errorf("hq_events16_encode_sized_multi: %d", int(rc))
	}
	return nil
}

// DeviceWire is the receiving side of a device worker (hq_wire_attach_device) with the framing on
// the device (hq_wire_set_device_framing): the transport hands over each received MessageBatch as
// it came, the host touches it once, to queue it, and Step frames, decodes, sorts and steps on the
// GPU.
type DeviceWire struct {
	w   *C.hq_wire
	x   *Worker
	out *C.hq_step_output // C memory
}

// OpenDeviceWire binds a wire of deploymentID to the device worker x.
func OpenDeviceWire(x *Worker, deploymentID uint64) (*DeviceWire, error) {
	d := &DeviceWire{x: x}
	if rc := C.hq_wire_open(C.uint64_t(deploymentID), &d.w); rc != C.HQ_OK {
		return nil, fmt.Errorf("hq_wire_open: %d", int(rc))
	}
	rc := C.hq_wire_attach_device(d.w, x.w)
	if rc == C.HQ_OK {
		rc = C.hq_wire_set_device_framing(d.w, 1)
	}
	if rc != C.HQ_OK {
		err := d.err(rc)
		C.hq_wire_close(d.w)
		return nil, err
	}
	d.out = (*C.hq_step_output)(C.calloc(1, C.size_t(unsafe.Sizeof(C.hq_step_output{}))))
	return d, nil
}

func (d *DeviceWire) err(rc C.int) error {
	if rc == C.HQ_OK {
		return nil
	}
	return fmt.Errorf("hipquorum wire error %d: %s", int(rc), C.GoString(C.hq_wire_last_error(d.w)))
}

// Close frees the wire (not the worker).
func (d *DeviceWire) Close() {
	C.hq_wire_close(d.w)
	C.free(unsafe.Pointer(d.out))
	d.w, d.out = nil, nil
}

// Reset starts a step.
func (d *DeviceWire) Reset() error { return d.err(C.hq_wire_reset(d.w)) }

// AddBatch queues one received MessageBatch. Pinned C memory is read by the device in place and
// must stay unchanged until Step returns; any other bytes are copied.
func (d *DeviceWire) AddBatch(b []byte) error {
	if len(b) == 0 {
		return d.err(C.hq_wire_add_batch(d.w, nil, 0))
	}
	var pin runtime.Pinner
	pin.Pin(&b[0])
	defer pin.Unpin()
	return d.err(C.hq_wire_add_batch(d.w, (*C.uint8_t)(unsafe.Pointer(&b[0])), C.size_t(len(b))))
}

// Step frames and decodes the queued batches on the device and steps the worker over them.
func (d *DeviceWire) Step() (*Output, error) {
	if rc := C.hq_wire_step_device(d.w, d.out, nil); rc != C.HQ_OK {
		return nil, d.err(rc)
	}
	return &Output{c: d.out}, nil
}

// Rejected lists the batches of the last Step that were dropped whole, for a framing error or a
// malformed message, as the indices of their AddBatch calls since Reset.
func (d *DeviceWire) Rejected() ([]uint32, error) {
	var p *C.uint32_t
	var n C.uint64_t
	if rc := C.hq_wire_device_rejected(d.w, &p, &n); rc != C.HQ_OK {
		return nil, d.err(rc)
	}
	if n == 0 {
		return nil, nil
	}
	return append([]uint32(nil), unsafe.Slice((*uint32)(unsafe.Pointer(p)), int(n))...), nil
}

// FrameStats is hq_wire_device_frame_stats: of the last Step the segments, the void segments and
// the batches that came back unconfirmed; and the steps framed on the host since the attach.
func (d *DeviceWire) FrameStats() (st [4]uint64, err error) {
	err = d.err(C.hq_wire_device_frame_stats(d.w, (*C.uint64_t)(unsafe.Pointer(&st[0]))))
	return st, err
}
