"""The drop-in scalar surface (agent.py) against the reference's recorded behaviour.

Re-authors the ten shipped unit tests (test_election.py, test_allocation.py) as exact
comparisons of everything each test observes -- state, leader, the positional _send_msg call
log and payload bytes -- plus four extra handler-corner scenarios, all recorded from the
reference by tools/gen_golden.py (tests/golden/scenarios.json).  CPU only."""
import json
import os
import struct
import time

import pytest

import agent
import scenarios
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "scenarios.json")) as f:
    RECORDED = json.load(f)


def _norm(x):
    return json.loads(json.dumps(x))


@pytest.mark.parametrize("fn", scenarios.ALL, ids=lambda f: f.__name__)
def test_scenario_matches_reference(fn):
    assert _norm(fn(agent)) == RECORDED[fn.__name__]


# The shipped assertions, restated directly (test_election.py:18-71, test_allocation.py:16-96).
def _agent(**kw):
    a = agent.SwarmAgent(**kw)
    a._send_msg = scenarios.Recorder()
    return a


def test_initial_state():
    a = _agent(agent_id=1, total_agents=3)
    assert a.state == agent.AgentState.FOLLOWER and a.leader_id is None


def test_election_timeout_trigger():
    a = _agent(agent_id=1, total_agents=3)
    a.last_heartbeat_time = time.time() - 5.0
    a._check_election_timeout()
    assert a.state == agent.AgentState.ELECTION_WAIT


def test_election_victory_after_wait():
    a = _agent(agent_id=1, total_agents=3)
    a.state = agent.AgentState.ELECTION_WAIT
    a.election_wait_start = time.time() - 1.0
    a.election_delay = 0.1
    a._check_election_timeout()
    assert a.state == agent.AgentState.LEADER and a.leader_id == 1
    sent = [c[0][0] for c in a._send_msg.calls]
    assert agent.MsgType.ELECTION_ACCLAIM in sent and agent.MsgType.COORDINATOR in sent


def test_bully_and_submit():
    a = _agent(agent_id=1, total_agents=3)
    a.state = agent.AgentState.LEADER
    a._handle_election_acclaim(sender=2)
    assert a.state == agent.AgentState.FOLLOWER and a.leader_id == 2
    b = _agent(agent_id=2, total_agents=3)
    b.state = agent.AgentState.LEADER
    b._handle_election_acclaim(sender=1)
    assert b.state == agent.AgentState.LEADER
    assert b._send_msg.calls[-1][0] == (agent.MsgType.HEARTBEAT, struct.pack("!ff", 0.0, 0.0))


def test_utility_and_claim():
    a = _agent(agent_id=1, total_agents=3, capabilities=["extinguisher"])
    assert a._calculate_utility({"status": "OPEN", "pos": (1.0, 0.0), "required_cap": "extinguisher"}) == 50.0
    assert a._calculate_utility({"status": "OPEN", "pos": (1.0, 0.0), "required_cap": "sonar"}) == 0.0
    a.tasks = {101: {"status": "OPEN", "pos": (1.0, 0.0), "required_cap": "extinguisher"}}
    a._process_tasks()
    mt, pl = a._send_msg.calls[-1][0]
    assert mt == agent.MsgType.TASK_CLAIM and struct.unpack("!If", pl) == (101, 50.0)


def test_conflict_resolution_and_hysteresis():
    a = _agent(agent_id=1, total_agents=3, capabilities=["extinguisher"])
    a.state = agent.AgentState.LEADER
    a._handle_task_claim(sender=2, payload=struct.pack("!If", 101, 50.0))
    assert a.task_claims[101]["winner"] == 2
    a._handle_task_claim(sender=3, payload=struct.pack("!If", 101, 52.0))
    assert a.task_claims[101]["winner"] == 2
    assert struct.unpack("!IB", a._send_msg.calls[-1][0][1]) == (101, 2)
    a._handle_task_claim(sender=3, payload=struct.pack("!If", 101, 60.0))
    assert a.task_claims[101]["winner"] == 3
    assert struct.unpack("!IB", a._send_msg.calls[-1][0][1]) == (101, 3)


def test_wire_caps_ids_at_255():
    """The u8 wire fields raise for IDs > 255, as the reference's formats do (agent.py:240,322)."""
    a = agent.SwarmAgent(300, 400)
    a.state = agent.AgentState.ELECTION_WAIT
    a.election_wait_start = time.time() - 1.0
    with pytest.raises(struct.error):
        a._check_election_timeout()


def test_transport_hook_receives_packets():
    a = agent.SwarmAgent(7, 10)
    got = []
    a.transport = got.append
    a._send_heartbeat()
    assert got == [struct.pack("!BBI", 1, 7, 0) + struct.pack("!ff", 0.0, 0.0)]
